"""``fewbit.functional.cross_entropy`` and ``fewbit.CrossEntropyLoss`` on the GPU (fewbit_amd/xent.py): values and gradients against ``F.cross_entropy``
on the float64 copy of the same inputs within the derived bounds (tests/xent_harness.py), what the node saves, the dtypes under autocast, the in-place
backward, capture into a graph, the swap with ``map_module`` and the fallbacks."""
import pytest
import torch
import torch.nn.functional as F

import fewbit
from norm_harness import saved_by
from xent_harness import DTYPES, ROUNDING, U, bits, bound_lse, draw, within

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SHAPES = ((37, 1027), (5, 50265))


def problem(rows, width, dtype, ignored, salt=0):
    values, t, _ = draw(rows, width, dtype, 50 + salt)
    if ignored:
        t[1::3] = -100
    return values.to(DEV), t.to(DEV)


def torch64(x, t, reduction, grad_output):
    """F.cross_entropy and its gradient on the float64 copy, on the host; also the per-row lse and loss"""
    xd = x.detach().double().cpu().requires_grad_()
    tc = t.cpu()
    rows_loss = F.cross_entropy(xd, tc, reduction='none')
    want = F.cross_entropy(xd, tc, reduction=reduction)
    want.backward(grad_output.double().cpu())
    return want.detach(), xd.grad, torch.logsumexp(xd.detach(), 1), rows_loss.detach()


def rooms(x, t, lse64, rows_loss64, d64, grow64):
    """the bounds of the header for the per-row loss and the gradient (``grow64``: the gradient arriving at each row's loss)"""
    x64, tc = x.detach().double().cpu(), t.cpu()
    e = bound_lse(x.shape[1], lse64)
    kept = tc != -100
    xt = x64.gather(1, tc.clamp_min(0)[:, None])[:, 0]
    row = torch.where(kept, e + 4 * U * (lse64.abs() + xt.abs()), torch.zeros_like(e))
    rel, absolute = ROUNDING[x.dtype]
    p64 = torch.exp(x64 - lse64[:, None])
    grad = grow64.abs()[:, None] * (p64 * (e[:, None] + 160 * U) + 2 * U) + rel * d64.abs() + absolute
    return row, grad


@pytest.mark.parametrize('ignored', (False, True))
@pytest.mark.parametrize('reduction', ('mean', 'sum', 'none'))
@pytest.mark.parametrize('rows, width', SHAPES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_values_and_gradients_are_torchs_in_float64_within_the_bounds(dtype, rows, width, reduction, ignored):
    x, t = problem(rows, width, dtype, ignored)
    count = int((t != -100).sum())
    g = torch.Generator().manual_seed(rows)
    gy = (torch.randn(rows, generator=g) if reduction == 'none' else torch.tensor(1.5)).to(DEV)
    # what arrives at each row's loss, as the layer forms it: grad_output, times the fp32 1 / count for the mean
    arriving = gy.float().cpu() * (torch.tensor(float(count)).reciprocal() if reduction == 'mean' else 1.0)
    want, d64, lse64, rows_loss64 = torch64(x, t, reduction, arriving.double() * (count if reduction == 'mean' else 1.0))
    grow64 = arriving.double().expand(rows)
    row_room, grad_room = rooms(x, t, lse64, rows_loss64, d64, grow64)
    scale = 1.0 / count if reduction == 'mean' else 1.0
    summed = (row_room.sum() + rows * U * rows_loss64.abs().sum()) * scale + 2 * U * want.abs()
    for call in (lambda v: fewbit.functional.cross_entropy(v, t, reduction=reduction, out_dtype=torch.float32),
                 lambda v: fewbit.CrossEntropyLoss(reduction=reduction, out_dtype=torch.float32)(v, t)):
        leaf = x.clone().requires_grad_()
        loss = call(leaf)
        assert loss.dtype == torch.float32 and loss.shape == want.shape
        within(loss, want, row_room if reduction == 'none' else summed, 'loss')
        loss.backward(gy)
        assert leaf.grad.dtype == dtype and leaf.grad.shape == x.shape
        within(leaf.grad, d64, grad_room, 'gradient')
        assert not leaf.grad[t == -100].any()
    # the default dtype of the result is the input's: the fp32 value rounded once
    assert torch.equal(fewbit.functional.cross_entropy(x, t, reduction=reduction), loss.detach().to(dtype))


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_mean_over_no_row_is_nan_and_its_gradient_zero(dtype):
    x, _ = problem(6, 257, dtype, False)
    t = torch.full((6, ), -100, device=DEV)
    leaf = x.clone().requires_grad_()
    loss = fewbit.functional.cross_entropy(leaf, t)
    assert torch.isnan(loss) and torch.isnan(F.cross_entropy(x.float(), t))
    loss.backward()
    assert not leaf.grad.any()
    assert float(fewbit.functional.cross_entropy(x, t, reduction='sum')) == 0.0


def storages(tensors):
    return {s.untyped_storage().data_ptr(): s.untyped_storage().nbytes() for s in tensors}


def test_the_node_saves_the_input_itself_and_a_few_bytes_per_row():
    rows, width = 64, 1000
    x, t = problem(rows, width, torch.bfloat16, True)
    leaf = x.clone().requires_grad_()
    for reduction in ('mean', 'sum', 'none'):
        loss, saved = saved_by(lambda: fewbit.functional.cross_entropy(leaf, t, reduction=reduction, out_dtype=torch.float32))
        kept = storages(saved)
        assert leaf.untyped_storage().data_ptr() in kept, 'the input is saved as a copy'
        assert any(s.data_ptr() == leaf.data_ptr() and s.dtype == leaf.dtype for s in saved)
        extra = sum(n for p, n in kept.items() if p != leaf.untyped_storage().data_ptr())
        assert extra <= 16 * rows + 16, (reduction, extra)
        assert all(s.numel() <= rows for s in saved if s.data_ptr() != leaf.data_ptr())
    logits_bytes = rows * width * 2
    _, saved = saved_by(lambda: F.cross_entropy(leaf.float(), t))
    assert sum(storages(saved).values()) >= 2 * logits_bytes
    # a row-sliced view is taken as it is: what is saved is still the caller's storage
    wide = torch.randn(rows, width + 8, device=DEV).to(torch.bfloat16).requires_grad_()
    sliced = wide[:, :width]
    loss, saved = saved_by(lambda: fewbit.functional.cross_entropy(sliced, t))
    assert wide.untyped_storage().data_ptr() in storages(saved)
    loss.backward()
    # (both layouts start every row on a 16-byte boundary, so the rows are walked alike: the same bits)
    ref = sliced.detach().contiguous().requires_grad_()
    fewbit.functional.cross_entropy(ref, t).backward()
    assert torch.equal(wide.grad[:, :width], ref.grad) and not wide.grad[:, width:].any()


def test_autocast_gives_an_fp32_loss_and_a_bf16_gradient():
    rows, width = 37, 1027
    x, t = problem(rows, width, torch.bfloat16, True)
    want, d64, lse64, rows_loss64 = torch64(x, t, 'mean', torch.tensor(1.0))
    count = int((t != -100).sum())
    grow64 = torch.tensor(float(count)).reciprocal().double().expand(rows)
    row_room, grad_room = rooms(x, t, lse64, rows_loss64, d64, grow64)
    room = (row_room.sum() + rows * U * rows_loss64.abs().sum()) / count + 2 * U * want.abs()
    leaf = x.clone().requires_grad_()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        loss = fewbit.functional.cross_entropy(leaf, t)
        theirs = F.cross_entropy(x, t)
    assert loss.dtype == torch.float32 == theirs.dtype
    within(loss, want, room, 'loss under autocast')                     # (fp32 accuracy: far inside what a bf16 result could give)
    assert float(room) < 2.0**-10 * float(want.abs())
    loss.backward()
    assert leaf.grad.dtype == torch.bfloat16
    within(leaf.grad, d64, grad_room, 'gradient under autocast')
    other = x.clone().requires_grad_()
    outside = fewbit.functional.cross_entropy(other, t, out_dtype=torch.float32)
    outside.backward()
    assert outside.dtype == torch.float32 and torch.equal(outside, loss) and torch.equal(other.grad, leaf.grad)
    assert fewbit.functional.cross_entropy(x, t).dtype == torch.bfloat16


def test_no_grad_and_an_input_that_needs_no_gradient_build_no_node():
    x, t = problem(9, 257, torch.float16, False)
    want = fewbit.functional.cross_entropy(x.clone().requires_grad_(), t).detach()
    with torch.no_grad():
        loss, saved = saved_by(lambda: fewbit.functional.cross_entropy(x.clone().requires_grad_(), t))
    assert saved == [] and loss.grad_fn is None and not loss.requires_grad and torch.equal(loss, want)
    loss, saved = saved_by(lambda: fewbit.functional.cross_entropy(x, t))
    assert saved == [] and loss.grad_fn is None and not loss.requires_grad and torch.equal(loss, want)
    single = fewbit.functional.cross_entropy(x[0], t[0], reduction='none')                 # a 1-D input with a 0-d target
    assert single.shape == () and torch.equal(single, fewbit.functional.cross_entropy(x[:1], t[:1], reduction='none')[0])


@pytest.mark.parametrize('reduction', ('mean', 'none'))
@pytest.mark.parametrize('dtype', DTYPES)
def test_the_in_place_backward_returns_the_logits_storage_with_the_same_bits(dtype, reduction):
    rows, width = 11, 2049
    x, t = problem(rows, width, dtype, True)
    gy = torch.ones((), device=DEV) if reduction == 'mean' else torch.linspace(-1, 1, rows, device=DEV)
    ref = x.clone().requires_grad_()
    fewbit.functional.cross_entropy(ref, t, reduction=reduction, out_dtype=torch.float32).backward(gy)

    source = x.clone().requires_grad_()
    logits = source * 1                                     # (not a leaf: the hook sees the tensor the node returns)
    seen = []
    logits.register_hook(seen.append)
    loss = fewbit.CrossEntropyLoss(reduction=reduction, out_dtype=torch.float32, inplace_backward=True)(logits, t)
    loss.backward(gy, retain_graph=True)
    assert len(seen) == 1 and seen[0].untyped_storage().data_ptr() == logits.untyped_storage().data_ptr() and seen[0].data_ptr() == logits.data_ptr()
    assert torch.equal(bits(seen[0]), bits(ref.grad)) and torch.equal(bits(source.grad), bits(ref.grad))
    assert torch.equal(bits(logits.detach()), bits(ref.grad)), 'the logits hold their gradient now'
    with pytest.raises(RuntimeError, match='second backward'):
        loss.backward(gy, retain_graph=True)
    # without retain_graph torch itself refuses the second backward
    again = (x.clone().requires_grad_() * 1)
    loss = fewbit.functional.cross_entropy(again, t, reduction=reduction, inplace_backward=True)
    loss.backward(gy.to(loss.dtype))
    with pytest.raises(RuntimeError):
        loss.backward(gy.to(loss.dtype))


def test_forward_and_backward_are_captured_and_replayed_on_new_contents():
    rows, width = 37, 1027
    x, t = problem(rows, width, torch.bfloat16, True)
    static_x, static_t = x.clone().requires_grad_(), t.clone()

    def step():
        loss = fewbit.functional.cross_entropy(static_x, static_t, out_dtype=torch.float32)
        return loss, torch.autograd.grad(loss, static_x)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                              # one eager call
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                           # (a host synchronisation in here would end the capture with an error)
        loss, grad = step()
    for salt in (1, 2):
        new_x, new_t = problem(rows, width, torch.bfloat16, salt == 1, salt)
        with torch.no_grad():
            static_x.copy_(new_x)
            static_t.copy_(new_t)
        graph.replay()
        torch.cuda.synchronize()
        leaf = new_x.clone().requires_grad_()
        want = fewbit.functional.cross_entropy(leaf, new_t, out_dtype=torch.float32)
        want.backward()
        assert torch.equal(loss, want) and torch.equal(grad, leaf.grad), salt


def test_a_model_is_swapped_with_map_module_and_the_fallbacks_give_torchs_values():
    class Model(torch.nn.Module):
        def __init__(self, **kw):
            super().__init__()
            self.head, self.loss = torch.nn.Linear(16, 257), torch.nn.CrossEntropyLoss(**kw)

        def forward(self, h, t):
            return self.loss(self.head(h), t)

    torch.manual_seed(5)
    h = torch.randn(12, 16, device=DEV)
    t = torch.randint(0, 257, (12, ), device=DEV)
    t[3] = 7
    swap = lambda m, path: fewbit.CrossEntropyLoss.from_loss(m) if type(m) is torch.nn.CrossEntropyLoss else m
    model = Model(ignore_index=7).to(DEV)
    want = model(h, t)
    want.backward()
    want_grad = model.head.weight.grad.clone()
    model.zero_grad()
    fewbit.map_module(model, swap)
    assert type(model.loss) is fewbit.CrossEntropyLoss and model.loss.ignore_index == 7
    got = model(h, t)
    got.backward()
    assert float((got - want).abs()) <= 1e-5 and float((model.head.weight.grad - want_grad).abs().max()) <= 1e-5
    # weights and label smoothing: torch's values through the fallback, bit for bit
    w = (torch.rand(257, device=DEV) + 0.5)
    for kw in ({'weight': w}, {'label_smoothing': 0.1}, {'weight': w, 'label_smoothing': 0.2, 'reduction': 'sum'}):
        model = Model(**kw).to(DEV)
        want = model(h, t)
        fewbit.map_module(model, swap)
        assert type(model.loss) is fewbit.CrossEntropyLoss and torch.equal(model(h, t), want)
    x = torch.randn(4, 257, 3, device=DEV)
    t3 = torch.randint(0, 257, (4, 3), device=DEV)
    assert torch.equal(fewbit.functional.cross_entropy(x, t3), F.cross_entropy(x, t3))
    assert torch.equal(fewbit.functional.cross_entropy(x.double()[..., 0], t3[:, 0]), F.cross_entropy(x.double()[..., 0], t3[:, 0]))
