"""``fewbit.functional.rms_norm_linear_mx`` / ``fewbit.MXNormLinear`` with a ``residual`` on the GPU at 65 tokens, 64 -> (32, 96): ONE node with the bytes
of ``dropout_add`` followed by the call without a residual, what it keeps, the unchanged default call, ``eval()`` and a captured step."""
import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi_x, linear
from norm_harness import DEV, saved_by

pytestmark = pytest.mark.gpu
BF16, EPS, P = torch.bfloat16, 1e-5, 0.1


def problem():                                                              # -> [x, r, gamma, W0, W1, b0] on the GPU, the gradients fed into q, k and h
    g = torch.Generator().manual_seed(9)
    shapes = ((65, 64), (65, 64), (64, ), (32, 64), (96, 64), (32, ))
    leaves = [((1.0 if s == (64, ) else 0.0) + 0.5 * torch.randn(s, generator=g)).to(BF16).to(DEV).requires_grad_() for s in shapes]
    return leaves, [torch.randn(65, n, generator=g).to(BF16).to(DEV) for n in (32, 96, 64)]


def node(leaves, **more):
    x, r, gamma, w0, w1, b0 = leaves
    return fewbit.functional.rms_norm_linear_mx(x, gamma, (w0, w1), (b0, None), EPS, 'fp4', residual=r, **more)


def test_values_and_gradients_are_those_of_dropout_add_and_the_plain_call(monkeypatch):
    """The seeds: the node makes ONE draw S from torch's default generator (``linear._draw_seed``), read here by drawing after the same
    ``torch.manual_seed``; the cells take S, G_i takes S + 1 + i and the mask S + 1 + 2.  The composition makes two draws, ``dropout_add``'s first:
    it is handed S + 3, then S."""
    leaves, grads = problem()
    torch.manual_seed(3)
    seed = linear._draw_seed(None)
    torch.manual_seed(3)
    outs = node(leaves, p=P, prenorm=True)
    assert len(outs) == 3 and len({id(o.grad_fn) for o in outs}) == 1 and outs[0].grad_fn.name() == '_AddRMSNormLinearMXBackward'
    got = torch.autograd.grad(outs, leaves, grads)
    handed = iter((seed + 3, seed))
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: next(handed))
    x, r, gamma, w0, w1, b0 = leaves
    h = fewbit.functional.dropout_add(x, r, P)
    want_outs = (*fewbit.functional.rms_norm_linear_mx(h, gamma, (w0, w1), (b0, None), EPS, 'fp4'), h)
    want = torch.autograd.grad(want_outs, leaves, grads)
    assert 0 < int((h == r).sum()) < h.numel() // 4                         # (a mask was drawn)
    for name, a, b in zip(('q', 'k', 'h', 'dx', 'dr', 'dgamma', 'dW0', 'dW1', 'db0'), (*outs, *got), (*want_outs, *want)):
        assert torch.equal(a, b), name


def test_what_is_kept_and_the_default_call():
    leaves, _ = problem()
    x, _, gamma, w0, w1, b0 = leaves
    outs, saved = saved_by(lambda: node(leaves, p=P, prenorm=True))
    assert len(saved) == 5 and sorted(t.numel() for t in saved if t.dtype == torch.uint8) == [cabi_x.mx_bytes(65, 64, 'fp4')]    # cells, rstd, gamma, two weights
    assert sum(t.dtype == torch.float32 and t.shape == (65, ) for t in saved) == 1 and all(any(t is p for t in saved) for p in (gamma, w0, w1))
    assert len(outs) == 3 and not any(t.dtype == BF16 and t.numel() == x.numel() for t in saved)
    torch.manual_seed(3)
    seed = linear._draw_seed(None)
    torch.manual_seed(3)
    plain = fewbit.functional.rms_norm_linear_mx(x, gamma, (w0, w1), (b0, None), EPS, 'fp4')
    y = cabi_x.mx_rms_norm_forward(x.detach(), gamma.detach(), EPS, 'fp4', seed)[0]
    assert len(plain) == 2 and all(o.grad_fn.name() == '_RMSNormLinearMXBackward' for o in plain)
    assert torch.equal(plain[0], F.linear(y, w0, b0)) and torch.equal(plain[1], F.linear(y, w1))


def test_the_module_in_eval_gives_torchs_values():
    leaves, _ = problem()
    x, r = leaves[:2]
    module = fewbit.MXNormLinear(64, [(64, 32, True), (64, 96, False)], eps=EPS, device=DEV, dtype=BF16, p=P, prenorm=True).eval()
    outs = module(x, r)
    y = F.rms_norm(r + x, (64, ), module.weight, EPS)
    assert len(outs) == 3 and torch.equal(outs[2], r + x) and all(torch.equal(o, m(y)) for o, m in zip(outs, module.linears))
    assert all('RMSNormLinearMX' not in o.grad_fn.name() for o in outs)


def test_a_captured_step_draws_a_fresh_mask_on_every_replay():
    leaves, grads = problem()

    def step():
        outs = node(leaves, p=P, prenorm=True)
        return (outs[2], *torch.autograd.grad(outs, leaves, grads))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                            # the eager warm-up: the per-device replay counter exists from here on
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        results = step()
    dropped = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all(bool(t.isfinite().all()) for t in results)
        dropped.append(results[0] == leaves[1])
    assert 0 < int(dropped[0].sum()) < dropped[0].numel() // 4 and not torch.equal(dropped[0], dropped[1])
