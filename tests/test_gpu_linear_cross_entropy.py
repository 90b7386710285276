"""``fewbit.functional.linear_cross_entropy`` on the GPU (fewbit_amd/xent.py) against float64: ``F.cross_entropy(F.linear(x64, W64, b64), t)`` and its autograd
gradients on the values the dtype holds.

The bound is not tuned.  With err(.) the largest absolute deviation from float64 of the loss, dx, dW or db, for this path and for torch's own composition
``F.cross_entropy(F.linear(x, W, b).float(), t)`` on the GPU in the same dtype:  err_here <= 2 err_torch + (k + 1) r max|reference|.  Two GEMM summation
orders, the chunked and the whole one, land anywhere in the same envelope: the factor 2.  dW and db are rounded once per chunk as they run and once at the
end: k = the number of chunks for them, 0 for the loss and dx; r = the unit roundoff (2^-8 bf16, 2^-11 fp16, 2^-24 fp32) of the dtype the quantity is kept
in: the dtype of the returned loss for the loss, the dtype the GEMMs run in for the gradients."""
import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import xent

pytestmark = pytest.mark.gpu

ROUNDOFF = {torch.bfloat16: 2.0**-8, torch.float16: 2.0**-11, torch.float32: 2.0**-24}
SHAPES = ((1, 8, 11, 4), (37, 24, 257, 16), (37, 24, 257, 64), (40, 8, 2049, 8))


def draw(n, h, v, dtype, bias=True, lead=None):
    """x, W ~ U(-1, 1), scaled so that the logits stay in about +-8"""
    g = torch.Generator().manual_seed(n * v + h)
    x = (torch.rand(*(lead or (n, )), h, generator=g) * 2 - 1).to(dtype).cuda()
    w = ((torch.rand(v, h, generator=g) * 2 - 1) * 4 / h**0.5).to(dtype).cuda()
    b = (torch.rand(v, generator=g) * 2 - 1).to(dtype).cuda() if bias else None
    return x, w, b, torch.randint(0, v, lead or (n, ), generator=g).cuda()


def outcome(f, x, w, b, t, dtype=None, needs=(True, True, True), times=1.0):
    """(loss, dx, dW, db) of ``f`` on fresh leaves of ``dtype``"""
    leaves = [None if v is None else v.detach().to(dtype or v.dtype).requires_grad_(need) for v, need in zip((x, w, b), needs)]
    loss = f(*leaves, t)
    (loss * times).backward()
    return (loss.detach(), ) + tuple(None if v is None else v.grad for v in leaves)


def held(x, w, b, t, chunks, ours, theirs=None, rounding=None, **kw):
    """the bound of the module docstring on every quantity; prints and returns the ratios err_here / err_torch"""
    reduction = kw.pop('reduction', 'mean')
    theirs = theirs or (lambda x, w, b, t: F.cross_entropy(F.linear(x, w, b).float().reshape(-1, w.shape[0]), t.reshape(-1), reduction=reduction))
    want = outcome(lambda x, w, b, t: F.cross_entropy(F.linear(x, w, b), t.reshape(-1), reduction=reduction), x.reshape(-1, x.shape[-1]), w, b, t, torch.float64, **kw)
    here, torchs = outcome(ours, x, w, b, t, **kw), outcome(theirs, x, w, b, t, **kw)
    ratios = {}
    for name, k, a, c, ref in zip(('loss', 'dx', 'dW', 'db'), (0, 0, chunks, chunks), here, torchs, want):
        assert (a is None) == (c is None) == (ref is None), name
        if ref is not None:
            ref, r = ref.reshape(a.shape), ROUNDOFF[a.dtype if name == 'loss' else rounding or x.dtype]
            err_here, err_torch = float((a.double() - ref).abs().max()), float((c.double() - ref).abs().max())
            ratios[name] = err_here / err_torch if err_torch else 0.0
            assert err_here <= 2 * err_torch + (k + 1) * r * float(ref.abs().max()), (name, err_here, err_torch)
    print('err_here / err_torch:', ', '.join(f'{name} {ratio:.2f}' for name, ratio in ratios.items()))
    return here


@pytest.mark.parametrize('bias', (True, False))
@pytest.mark.parametrize('reduction', ('mean', 'sum'))
@pytest.mark.parametrize('n, h, v, chunk', SHAPES)
@pytest.mark.parametrize('dtype', (torch.float32, torch.float16, torch.bfloat16))
def test_the_loss_and_the_three_gradients_are_float64s(dtype, n, h, v, chunk, reduction, bias):
    x, w, b, t = draw(n, h, v, dtype, bias)
    if n > 1:                                                                        # (a lone row stays: the mean of no row is NaN)
        t[n // 2] = -100
    ours = lambda x, w, b, t: fewbit.functional.linear_cross_entropy(x, w, t, b, reduction=reduction, chunk_rows=chunk)
    loss, dx, dw, db = held(x, w, b, t, -(-n // chunk), ours, reduction=reduction)
    assert loss.dtype == dx.dtype == dw.dtype == dtype and dx.shape == x.shape and dw.shape == w.shape and (db is None) == (not bias)


def test_ignored_chunks_frozen_operands_more_dimensions_and_a_scaled_loss():
    x, w, b, t = draw(37, 24, 257, torch.bfloat16)
    module = fewbit.LinearCrossEntropyLoss(chunk_rows=16)
    ours = lambda x, w, b, t: module(x, w, t, b)
    t[16:32] = -100                                                                  # a whole chunk of ignored targets
    held(x, w, b, t, 3, ours, times=3.0)                                             # ... and loss * 3
    _, dx, dw, db = held(x, w, b, t, 3, ours, needs=(True, False, True))             # the weight frozen
    assert dw is None and dx is not None and db is not None
    _, dx, dw, db = held(x, w, b, t, 3, ours, needs=(False, True, False))            # the input and the bias frozen
    assert dx is None and db is None and dw is not None
    held(x, w, b, t, 3, lambda x, w, b, t: fewbit.functional.linear_cross_entropy(x, w, t, b, chunk_rows=16, accumulate_dtype=torch.float32))
    t[:] = -100                                                                      # all ignored: the mean of no row, as torch
    loss, dx, dw, db = outcome(ours, x, w, b, t)
    assert torch.isnan(loss) and not dx.any() and not dw.any() and not db.any()
    x, w, b, t = draw(10, 8, 2049, torch.bfloat16, lead=(2, 5))                      # a 3-D input, targets of its shape
    _, dx, _, _ = held(x, w, b, t, 2, lambda x, w, b, t: fewbit.functional.linear_cross_entropy(x, w, t, b, chunk_rows=8, reduction='sum'), reduction='sum')
    assert dx.shape == (2, 5, 8)


def test_under_autocast_fp32_parameters_give_an_fp32_loss_and_fp32_gradients():
    x, w, b, t = draw(37, 24, 257, torch.float32)

    def under(f):
        def run(*args):
            with torch.autocast('cuda', dtype=torch.bfloat16):
                return f(*args)
        return run

    ours = under(lambda x, w, b, t: fewbit.functional.linear_cross_entropy(x, w, t, b, chunk_rows=16))
    loss, dx, dw, db = held(x, w, b, t, 3, ours, under(lambda x, w, b, t: F.cross_entropy(F.linear(x, w, b), t)), rounding=torch.bfloat16)
    assert loss.dtype == dx.dtype == dw.dtype == db.dtype == torch.float32


def test_a_second_backward_raises():
    x, w, b, t = draw(37, 24, 257, torch.bfloat16)
    x.requires_grad_()
    loss = fewbit.functional.linear_cross_entropy(x, w, t, b, chunk_rows=16)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second backward'):
        loss.backward()


def test_a_captured_call_replays_to_the_bits_of_the_eager_call():
    x, w, b, t = draw(37, 24, 257, torch.bfloat16)
    f = lambda x, w, b, t: fewbit.functional.linear_cross_entropy(x, w, t, b, chunk_rows=16)
    eager = outcome(f, x, w, b, t)
    leaves = [v.clone().requires_grad_() for v in (x, w, b)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                    # (torch's recipe: warm up on a side stream, then capture)
        f(*leaves, t).backward()
    torch.cuda.current_stream().wait_stream(side)
    for v in leaves:
        v.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = f(*leaves, t)
        loss.backward()
    for _ in range(3):
        loss.fill_(7.0)
        for v in leaves:
            v.grad.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        for a, c in zip((loss, *(v.grad for v in leaves)), eager):
            assert torch.equal(a.view(torch.int16), c.view(torch.int16))


def test_the_allocators_peak_stays_below_one_logits_tensor():
    n, h, v, chunk = 2048, 64, 8192, 256
    x, w, b, t = draw(n, h, v, torch.bfloat16, bias=False)
    assert xent.default_chunk_rows(n, h, v) == n                                     # (the default would be one chunk: the logits whole)
    f = lambda: outcome(lambda x, w, b, t: fewbit.functional.linear_cross_entropy(x, w, t, chunk_rows=chunk), x, w, b, t)
    f()                                                                              # (the GEMM workspace exists from here on)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    f()
    peak = torch.cuda.max_memory_allocated() - before
    print(f'peak {peak} bytes, one logits tensor {n * v * 2} bytes')
    assert peak < n * v * 2
