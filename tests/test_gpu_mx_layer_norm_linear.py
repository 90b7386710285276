"""``fewbit.MXLayerNormLinear`` / ``fewbit.functional.layer_norm_linear_mx`` on the GPU at 65 tokens, width -> (96 with bias, 32), with
``return_normed=True`` and a random gradient at ``y``: the outputs bit for bit from the norm kernel's ``y``, what is kept, and every gradient against a
float64 evaluation of the composition on the same values, by the criterion of tests/test_gpu_mx_norm_linear.py: a weight gradient may be
1.5 sqrt(host^2 + 0.037^2) off (host: the host route's error with the same seed, 0.037 the recorded fp8-gradient term), dx and dgamma 1.5 host, floored
at the dtype's unit.  dbeta carries no rounding of cells: at most twice the error of the plain torch composition on the same device and dtype, floored at
the dtype's unit.  beta ~ N(0, 1), so that a node which forgets ``s (x) beta`` in a weight gradient fails by a wide margin.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi_x
from norm_harness import DEV, UNIT, saved_by

pytestmark = pytest.mark.gpu
NAMES = ('dx', 'dgamma', 'dbeta', 'dW0', 'dW1')
OUT = (96, 32)


def problem(format, dtype, width=64):
    torch.manual_seed(5)
    module = fewbit.MXLayerNormLinear(width, [(width, 96, True), (width, 32, False)], format=format, return_normed=True, dtype=dtype)
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        module.weight.copy_(1 + 0.5 * torch.randn(width, generator=gen))
        module.bias.copy_(torch.randn(width, generator=gen))
    return module, torch.randn(65, width, generator=gen).to(dtype), [torch.randn(65, n, generator=gen).to(dtype) for n in (width, *OUT)]


def leaves(module):
    return (module.weight, module.bias, *(m.weight for m in module.linears), module.linears[0].bias)


def gradients(module, x, grads, device, plain=False):
    """-> (outputs, [dx, dgamma, dbeta, dW0, dW1, db0]) of a copy of ``module`` on ``device``, every rounding seeded by generator seed 21; ``plain``:
    of the torch composition (the module in eval mode) instead"""
    module = copy.deepcopy(module).to(device).train(not plain)
    module.generator = torch.Generator().manual_seed(21)
    x = x.to(device).requires_grad_()
    outs = module(x)
    return outs, torch.autograd.grad(outs, (x, *leaves(module)), [g.to(device) for g in grads])


def errors(got, module, x, grads):
    x64, (gamma, beta, *weights, _) = x.double().requires_grad_(), [p.detach().double().requires_grad_() for p in leaves(module)]
    y = F.layer_norm(x64, (x.shape[1], ), gamma, beta, 1e-5)
    want = torch.autograd.grad([y] + [F.linear(y, w) for w in weights], (x64, gamma, beta, *weights), [g.double() for g in grads])
    return [float((a.detach().cpu().double() - b).norm() / b.norm()) for a, b in zip(got, want)]


@pytest.mark.parametrize('width', (64, 72), ids=('mx_wgrad', 'decode_route'))
@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float32), ids=('bf16', 'fp32'))
@pytest.mark.parametrize('format', ('fp4', 'fp6'))
def test_outputs_are_the_kernels_and_the_gradients_hold_the_host_routes_bound(format, dtype, width, monkeypatch):
    calls = []
    real = cabi_x.mx_wgrad
    monkeypatch.setattr(cabi_x, 'mx_wgrad', lambda *a, **k: calls.append(a[3:5]) or real(*a, **k))
    module, x, grads = problem(format, dtype, width)
    outs, got = gradients(module, x, grads, DEV)
    on = copy.deepcopy(module).to(DEV)
    y = cabi_x.mx_layer_norm_forward(x.to(DEV), on.weight.detach(), on.bias.detach(), 1e-5, format, 0)[0]
    assert all(out.grad_fn.name() == '_LayerNormLinearMXBackward' for out in outs) and torch.equal(outs[0], y)
    assert all(torch.equal(out, m(y)) for out, m in zip(outs[1:], on.linears))
    assert calls == ([(64, n) for n in OUT] if width == 64 else []) and torch.equal(got[5], grads[1].to(DEV).sum(dim=0))
    gpu, host = errors(got[:5], module, x, grads), errors(gradients(module, x, grads, 'cpu')[1][:5], module, x, grads)
    torch_dbeta = errors(gradients(module, x, grads, DEV, plain=True)[1][:5], module, x, grads)[2]
    print(f'{format} {dtype} width {width}: relative errors against float64 of {NAMES}: kernels {[round(e, 5) for e in gpu]}, host route '
          f'{[round(e, 5) for e in host]}; dbeta of the torch composition {torch_dbeta:.3g}')
    for name, g, h in zip(NAMES, gpu, host):
        allowed = (2.0 * max(torch_dbeta, UNIT[dtype]) if name == 'dbeta' else 1.5 * max(h, UNIT[dtype]) if name in ('dx', 'dgamma')
                   else 1.5 * (h * h + 0.037**2)**0.5)
        assert g <= allowed, (name, g, h, allowed)


def test_what_is_kept_what_builds_no_node_and_from_modules():
    module, x, _ = problem('fp4', torch.bfloat16)
    module, xd = module.to(DEV), x.to(DEV).requires_grad_()
    outs, saved = saved_by(lambda: module(xd))
    weights = [m.weight for m in module.linears]
    assert sorted(t.numel() for t in saved if t.dtype == torch.uint8) == [cabi_x.mx_bytes(65, 64, 'fp4')] and len(saved) == 6    # cells, rstd, gamma, beta, two weights
    assert sum(t.dtype == torch.float32 and t.shape == (65, ) for t in saved) == 1 and all(any(t is p for t in saved) for p in (module.weight, module.bias, *weights))
    with torch.no_grad():
        plain, nothing = saved_by(lambda: module(xd))
    assert all(p.grad_fn is None for p in plain) and not nothing and len(plain) == 3
    exact = module.eval()(xd)
    assert len(exact) == 3 and all('LayerNormLinearMX' not in out.grad_fn.name() for out in exact)
    norm = torch.nn.LayerNorm(64, eps=1e-12, device=DEV, dtype=torch.bfloat16)
    swapped = fewbit.MXLayerNormLinear.from_modules(norm, list(module.linears), format='fp6', return_normed=True)
    assert swapped.weight is norm.weight and swapped.bias is norm.bias and all(a is b for a, b in zip(swapped.linears, module.linears))
    assert (swapped.eps, swapped.format, swapped.return_normed, swapped.training) == (1e-12, 'fp6', True, True)
