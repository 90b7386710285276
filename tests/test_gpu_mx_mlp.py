"""``fewbit.MXMLP`` / ``fewbit.functional.mlp_mx`` on the GPU at 96 tokens, 64 -> 96 -> 64, bf16: the output, the four gradients against a float64 MLP on
the same values, what is kept and what is skipped (the shape of tests/test_gpu_mx_gated_mlp.py).

The output is ``fc2(mx_act_forward(fc1(x))[0])`` bit for bit.  The bound of the gradients is that test's: the node's host route (CPU tensors, the same
generator seed) rounds no gradient to fp8; with its relative Frobenius errors ``h`` against the same float64 reference, the kernels' route may be at
most ``1.5 * sqrt(h^2 + 0.037^2)`` -- 0.037 the measured error of an fp8 gradient (EXPERIMENTS.md 8.32), 1.5 the spread of one seed.  The composed route
on the device (an intermediate width of 40) rounds what the host route rounds: at most ``1.5 h`` of a host run of its own.
MEASURED on an MI355X (EXPERIMENTS.md 8.36): the figures the tests print."""
import copy

import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi_x
from norm_harness import DEV, saved_by

pytestmark = pytest.mark.gpu
NAMES = ('dx', 'dW1', 'db1', 'dW2')


def problem(format, activation, intermediate=96):
    torch.manual_seed(5)
    mlp = fewbit.MXMLP(64, intermediate, activation=activation, format=format, dtype=torch.bfloat16)
    gen = torch.Generator().manual_seed(9)
    return mlp, torch.randn(96, 64, generator=gen).bfloat16(), torch.randn(96, 64, generator=gen).bfloat16()


def gradients(mlp, x, gy, device):
    """-> (output, [dx, dW1, db1, dW2]) of a copy of ``mlp`` on ``device``, every rounding seeded by generator seed 21"""
    mlp = copy.deepcopy(mlp).to(device)
    mlp.generator = torch.Generator().manual_seed(21)
    x = x.to(device).requires_grad_()
    out = mlp(x)
    return out, torch.autograd.grad(out, (x, mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight), gy.to(device))


def errors(got, mlp, x, gy):
    act = {'relu': F.relu, 'silu': F.silu, 'gelu': F.gelu, 'gelu_tanh': lambda t: F.gelu(t, approximate='tanh')}[mlp.activation]
    x64, (w1, b1, w2, b2) = x.double().requires_grad_(), [p.detach().double().requires_grad_() for p in (mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias)]
    want = torch.autograd.grad(F.linear(act(F.linear(x64, w1, b1)), w2, b2), (x64, w1, b1, w2), gy.double())
    return [float((a.detach().cpu().double() - b).norm() / b.norm()) for a, b in zip(got, want)]


@pytest.mark.parametrize('activation', cabi_x.MX_ACTIVATIONS)
@pytest.mark.parametrize('format', ('fp4', 'fp6'))
def test_the_output_is_the_kernels_and_the_gradients_hold_the_host_routes_bound(format, activation):
    mlp, x, gy = problem(format, activation)
    out, got = gradients(mlp, x, gy, DEV)
    on = copy.deepcopy(mlp).to(DEV)
    assert out.grad_fn.name() == '_MLPMXBackward' and torch.equal(out, on.fc2(cabi_x.mx_act_forward(on.fc1(x.to(DEV)), activation, format, keep=False)[0]))
    gpu, host = errors(got, mlp, x, gy), errors(gradients(mlp, x, gy, 'cpu')[1], mlp, x, gy)
    print(f'{format} {activation}: relative errors against float64 of {NAMES}: kernels {[round(e, 4) for e in gpu]}, host route {[round(e, 4) for e in host]}')
    for name, g, h in zip(NAMES, gpu, host):
        assert g <= 1.5 * (h * h + 0.037**2)**0.5, (name, g, h)


def test_what_is_kept_what_is_skipped_the_composed_route_and_from_linears(monkeypatch):
    mlp, x, gy = problem('fp6', 'gelu')
    mlp, xd = mlp.to(DEV), x.to(DEV).requires_grad_()
    out, saved = saved_by(lambda: mlp(xd))
    kept = sorted(t.numel() for t in saved if t.dtype == torch.uint8)
    assert kept == sorted((cabi_x.mx_bytes(96, 64, 'fp6'), cabi_x.mx_bytes(96, 96, 'fp6'))) and len(saved) == 4       # x^, u^, two weights
    # no_grad keeps nothing and is the same bytes; a frozen fc2.weight skips its mx_wgrad and the pack of grad_output
    with torch.no_grad():
        plain, nothing = saved_by(lambda: mlp(xd))
    assert plain.grad_fn is None and not nothing and torch.equal(plain, out)
    calls, packs = [], []
    real, real_pack = cabi_x.mx_wgrad, cabi_x.mx_pack
    monkeypatch.setattr(cabi_x, 'mx_wgrad', lambda *a, **k: calls.append(a[3:5]) or real(*a, **k))
    monkeypatch.setattr(cabi_x, 'mx_pack', lambda *a, **k: packs.append(a[2:]) or real_pack(*a, **k))
    mlp.fc2.weight.requires_grad_(False)
    grads = torch.autograd.grad(mlp(xd), (xd, mlp.fc1.weight, mlp.fc1.bias), gy.to(DEV))
    assert calls == [(64, 96)] and packs == [('fp6', 'kept')] and all(bool(torch.isfinite(g).all()) for g in grads)      # (the one pack: x in forward)
    # an intermediate width of 40: no kernel of mx_wgrad, the composed route on the device
    narrow, x, gy = problem('fp6', 'gelu', 40)
    del calls[:]
    gpu, host = errors(gradients(narrow, x, gy, DEV)[1], narrow, x, gy), errors(gradients(narrow, x, gy, 'cpu')[1], narrow, x, gy)
    print(f'intermediate 40: composed on the device {[round(e, 4) for e in gpu]}, host route {[round(e, 4) for e in host]}')
    assert not calls and all(g <= 1.5 * h for g, h in zip(gpu, host))
    # from_linears shares both layers
    shared = fewbit.MXMLP.from_linears(mlp.fc1, mlp.fc2, activation='relu', format='fp4')
    assert shared.fc1 is mlp.fc1 and shared.fc2 is mlp.fc2 and (shared.activation, shared.format) == ('relu', 'fp4')
