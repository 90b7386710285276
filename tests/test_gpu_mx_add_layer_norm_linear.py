"""``fewbit.functional.layer_norm_linear_mx`` / ``fewbit.MXLayerNormLinear`` with a ``residual`` on the GPU at 65 tokens, 64 -> (96, 32): ONE node with
the bytes of ``dropout_add`` followed by the call without a residual, what it keeps, autocast, a gradient at ``y`` alone, and the composed width."""
import pytest
import torch

import fewbit
from fewbit_amd import cabi_x, linear
from norm_harness import DEV, saved_by

pytestmark = pytest.mark.gpu
EPS, P = 1e-5, 0.1
dtypes = pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float16), ids=('bf16', 'fp16'))


def problem(dtype, width=64):                                               # -> the module, x, r on the GPU, the gradients fed into y, the linears and h
    g = torch.Generator().manual_seed(9)
    module = fewbit.MXLayerNormLinear(width, [(width, 96, True), (width, 32, False)], eps=EPS, device=DEV, dtype=dtype, p=P, return_normed=True)
    with torch.no_grad():
        for q in module.parameters():
            q.copy_(((1.0 if q is module.weight else 0.0) + 0.5 * torch.randn(q.shape, generator=g)).to(dtype))
    x, r = (torch.randn(65, width, generator=g).to(dtype).to(DEV).requires_grad_() for _ in range(2))
    return module, x, r, [torch.randn(65, n, generator=g).to(dtype).to(DEV) for n in (width, 96, 32, width)]


@dtypes
@pytest.mark.parametrize('prenorm', (False, True))
def test_values_and_gradients_are_those_of_dropout_add_and_the_plain_call(monkeypatch, dtype, prenorm):
    """The seeds: the node makes ONE draw S (``linear._draw_seed``), read here by drawing after the same ``torch.manual_seed``; the cells take S, G_i
    takes S + 1 + i and the mask S + 1 + 2.  The composition makes two draws, ``dropout_add``'s first: it is handed S + 3, then S."""
    module, x, r, grads = problem(dtype)
    module.prenorm, grads = prenorm, grads[:4 if prenorm else 3]
    leaves = (x, r, *module.parameters())
    torch.manual_seed(3)
    seed = linear._draw_seed(None)
    torch.manual_seed(3)
    outs = module(x, r)
    assert len(outs) == len(grads) and len({id(o.grad_fn) for o in outs}) == 1 and outs[0].grad_fn.name() == '_AddLayerNormLinearMXBackward'
    got = torch.autograd.grad(outs, leaves, grads)
    handed = iter((seed + 3, seed))
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: next(handed))
    h = fewbit.functional.dropout_add(x, r, P)
    weights, biases = [m.weight for m in module.linears], [m.bias for m in module.linears]
    want_outs = fewbit.functional.layer_norm_linear_mx(h, module.weight, module.bias, weights, biases, EPS, 'fp4', return_normed=True) + ((h, ) if prenorm else ())
    want = torch.autograd.grad(want_outs, leaves, grads)
    assert 0 < int((h == r).sum()) < h.numel() // 4                         # (a mask was drawn)
    assert all(torch.equal(a, b) for a, b in zip((*outs, *got), (*want_outs, *want)))


def test_what_is_kept_autocast_and_a_gradient_at_y_alone():
    module, x, r, grads = problem(torch.bfloat16)
    outs, saved = saved_by(lambda: module(x, r))
    assert len(saved) == 6 and sorted(t.numel() for t in saved if t.dtype == torch.uint8) == [cabi_x.mx_bytes(65, 64, 'fp4')]  # cells, rstd, gamma, beta, weights
    assert not any(t.numel() == x.numel() and t.dtype != torch.uint8 for t in saved)
    dx, dr, dgamma = torch.autograd.grad(module(x, r)[0], (x, r, module.weight), grads[0])     # only y has a gradient: it is gy itself
    assert all(bool(t.isfinite().all()) for t in (dx, dr, dgamma)) and torch.equal(dx == 0, (dx == 0) | (dr == 0)) and 0 < int((dx == 0).sum()) < dx.numel() // 4
    with torch.autocast('cuda', dtype=torch.bfloat16):
        y, a, b = module(x.float().detach().requires_grad_(), r.float())
    assert y.dtype == torch.float32 and a.dtype == torch.bfloat16 and a.grad_fn.name() == '_AddLayerNormLinearMXBackward'
    (a.float().sum() + b.float().sum() + y.sum()).backward()
    assert all(q.grad is not None and bool(q.grad.isfinite().all()) for q in module.parameters())


def test_a_mask_at_width_13_runs_as_the_composition():
    module, x, r, grads = problem(torch.bfloat16, 13)
    outs = module(x, r)
    assert outs[0].grad_fn.name() == '_LayerNormLinearMXBackward' and len(outs) == 3
    assert all(bool(t.isfinite().all()) for t in torch.autograd.grad(outs, (x, r), grads[:3]))
