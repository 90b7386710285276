"""``fewbit.MXGatedMLP`` / ``fewbit.functional.gated_mlp_mx`` on the GPU at 96 tokens, 64 -> 96 -> 64, bf16: the output, the four gradients against a
float64 MLP on the same values, what is kept and what is skipped.

The output: "the plain MLP" is this package's plain forward -- torch's three GEMMs around the product kernel, which evaluates ``act`` in fp32 and
rounds ONE product (torch's own ``act(gate) * up`` rounds ``act(gate)`` to bf16 first and differs in the last bit); the node's output is that, bit for bit.

The bound of the gradients is not fixed in advance: the node's host route (CPU tensors, the same generator seed, the same seven seeds) rounds no
gradient to fp8; with its four relative Frobenius errors ``h`` against the same float64 reference, the kernels' route may be at most
``1.5 * sqrt(h^2 + 0.037^2)`` -- 0.037 the measured error of an fp8 gradient (EXPERIMENTS.md 8.32), 1.5 the spread of one seed.  The composed route on
the device (an intermediate width of 40) rounds what the host route rounds: at most ``1.5 h`` of a host run of its own.
MEASURED on an MI355X (EXPERIMENTS.md 8.33): the figures the tests print."""
import copy

import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi_x
from norm_harness import DEV, saved_by

pytestmark = pytest.mark.gpu
NAMES = ('dx', 'dWg', 'dWu', 'dWd')


def problem(format, activation, intermediate=96):
    torch.manual_seed(5)
    mlp = fewbit.MXGatedMLP(64, intermediate, activation=activation, format=format, dtype=torch.bfloat16)
    gen = torch.Generator().manual_seed(9)
    return mlp, torch.randn(96, 64, generator=gen).bfloat16(), torch.randn(96, 64, generator=gen).bfloat16()


def gradients(mlp, x, gy, device):
    """-> (output, [dx, dWg, dWu, dWd]) of a copy of ``mlp`` on ``device``, every rounding seeded by generator seed 21"""
    mlp = copy.deepcopy(mlp).to(device)
    mlp.generator = torch.Generator().manual_seed(21)
    x = x.to(device).requires_grad_()
    out = mlp(x)
    return out, torch.autograd.grad(out, (x, mlp.gate_proj.weight, mlp.up_proj.weight, mlp.down_proj.weight), gy.to(device))


def errors(got, mlp, x, gy):
    act = F.silu if mlp.activation == 'silu' else F.gelu
    x64, (wg, wu, wd) = x.double().requires_grad_(), [p.detach().double().requires_grad_() for p in (mlp.gate_proj.weight, mlp.up_proj.weight, mlp.down_proj.weight)]
    want = torch.autograd.grad(F.linear(act(F.linear(x64, wg)) * F.linear(x64, wu), wd), (x64, wg, wu, wd), gy.double())
    return [float((a.detach().cpu().double() - b).norm() / b.norm()) for a, b in zip(got, want)]


@pytest.mark.parametrize('activation', ('silu', 'gelu'))
@pytest.mark.parametrize('format', ('fp4', 'fp6'))
def test_the_output_is_the_plain_mlps_and_the_gradients_hold_the_host_routes_bound(format, activation):
    mlp, x, gy = problem(format, activation)
    out, got = gradients(mlp, x, gy, DEV)
    on = copy.deepcopy(mlp).to(DEV)
    product = cabi_x.glu_forward(on.gate_proj(x.to(DEV)), on.up_proj(x.to(DEV)), activation, keep=False)[0]
    assert out.grad_fn.name() == '_GatedMLPMXBackward' and torch.equal(out, on.down_proj(product))
    gpu, host = errors(got, mlp, x, gy), errors(gradients(mlp, x, gy, 'cpu')[1], mlp, x, gy)
    print(f'{format} {activation}: relative errors against float64 of {NAMES}: kernels {[round(e, 4) for e in gpu]}, host route {[round(e, 4) for e in host]}')
    for name, g, h in zip(NAMES, gpu, host):
        assert g <= 1.5 * (h * h + 0.037**2)**0.5, (name, g, h)


def test_what_is_kept_what_is_skipped_the_composed_route_and_from_mlp(monkeypatch):
    mlp, x, gy = problem('fp6', 'silu')
    mlp, xd = mlp.to(DEV), x.to(DEV).requires_grad_()
    out, saved = saved_by(lambda: mlp(xd))
    kept = sorted(t.numel() for t in saved if t.dtype == torch.uint8)
    assert kept == sorted((cabi_x.mx_bytes(96, 64, 'fp6'), cabi_x.mx_glu_state_bytes(96, 96, 'fp6'))) and len(saved) == 5      # x^, the state, three weights
    # no_grad keeps nothing and is the same bytes; a frozen down_proj skips its product (and the pack of grad_output)
    with torch.no_grad():
        plain, nothing = saved_by(lambda: mlp(xd))
    assert plain.grad_fn is None and not nothing and torch.equal(plain, out)
    calls = []
    real = cabi_x.mx_wgrad
    monkeypatch.setattr(cabi_x, 'mx_wgrad', lambda *a, **k: calls.append(a[3:5]) or real(*a, **k))
    mlp.down_proj.weight.requires_grad_(False)
    grads = torch.autograd.grad(mlp(xd), (xd, mlp.gate_proj.weight, mlp.up_proj.weight), gy.to(DEV))
    assert calls == [(64, 96), (64, 96)] and all(bool(torch.isfinite(g).all()) for g in grads)
    # an intermediate width of 40: no kernel of mx_wgrad, the composed route on the device
    narrow, x, gy = problem('fp6', 'silu', 40)
    del calls[:]
    gpu, host = errors(gradients(narrow, x, gy, DEV)[1], narrow, x, gy), errors(gradients(narrow, x, gy, 'cpu')[1], narrow, x, gy)
    print(f'intermediate 40: composed on the device {[round(e, 4) for e in gpu]}, host route {[round(e, 4) for e in host]}')
    assert not calls and all(g <= 1.5 * h for g, h in zip(gpu, host))
    # from_mlp shares the three projections and reads act_fn
    llama = torch.nn.Module()
    llama.gate_proj, llama.up_proj, llama.down_proj, llama.act_fn = mlp.gate_proj, mlp.up_proj, mlp.down_proj, torch.nn.GELU()
    swapped = fewbit.MXGatedMLP.from_mlp(llama, format='fp4')
    assert swapped.gate_proj is mlp.gate_proj and swapped.up_proj is mlp.up_proj and swapped.down_proj is mlp.down_proj
    assert (swapped.activation, swapped.format) == ('gelu', 'fp4')
