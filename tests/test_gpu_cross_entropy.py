"""The cross-entropy entry points of the companion library on the GPU (include/fewbit_hipx.h, "The loss of a row"; fewbit_amd/csrc/fewbit_xent.hip), at
the binding level: every lse, loss and gradient against the float64 host evaluation within the derived bounds of the header (tests/xent_harness.py),
on rows that start on no 16-byte boundary, with -inf logits, NaN rows, ignored and out-of-range targets, in place, and beyond the caps of the plan."""
import math
import re
from pathlib import Path

import pytest
import torch

from fewbit_amd import cabi_x
from xent_harness import DTYPES, U, Placed, bits, check, draw

pytestmark = pytest.mark.gpu

INF = float('inf')
# around the block of eight, the wave, one sweep of the workgroup (256 pieces: 2048 16-bit elements), and odd: rows fall on every alignment
WIDTHS = (1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4099)


def run(placed, t, grow, ignore_index=-100, out=None):
    """forward and backward of the placed logits -> (lse, loss, the output's Placed)"""
    t = t.to(placed.view.device)
    lse, loss = cabi_x.cross_entropy_forward(placed.view, t, ignore_index)
    out = placed.empty_like() if out is None else out
    cabi_x.cross_entropy_backward(placed.view, t, lse, grow.to(placed.view.device), ignore_index, out=out.view)
    return lse, loss, out


def run_and_check(values, t, grow, ld=None, ignore_index=-100, offset=1):
    placed = Placed(values, ld, offset)
    lse, loss, out = run(placed, t, grow, ignore_index)
    worst = check(placed.view, t, grow, lse, loss, out.view, ignore_index)
    assert placed.untouched() and out.untouched(), 'something outside the rows was written'
    assert torch.equal(bits(placed.view.cpu()), bits(values)), 'the logits were changed'
    return placed, lse, loss, out, worst


@pytest.mark.parametrize('width', WIDTHS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_every_lse_loss_and_gradient_is_inside_its_bound(dtype, width):
    worst = [0.0, 0.0, 0.0]
    for rows in (1, 3, 5):
        for ld in (width, width + 3):
            values, t, grow = draw(rows, width, dtype, rows)
            placed, lse, loss, out, w = run_and_check(values, t, grow, ld)
            worst = [max(a, b) for a, b in zip(worst, w)]
            # an output at another offset from the 16-byte boundary (the element-wise stores): the same bytes
            other = placed.empty_like(offset=3, ld=width + 1)
            run(placed, t, grow, out=other)
            assert torch.equal(bits(other.view), bits(out.view)) and other.untouched()
    print(f'{dtype} width {width}: worst fractions of the bounds (lse, loss, dlogits) = {worst[0]:.3f}, {worst[1]:.3f}, {worst[2]:.3f}')


@pytest.mark.parametrize('width', (65, 257, 600))
@pytest.mark.parametrize('dtype', DTYPES)
def test_every_position_is_read_once_and_written_once(dtype, width):
    """-16 everywhere, +16 on the diagonal: a skipped or doubly read position moves lse or a gradient by order 1"""
    values = torch.full((width, width), -16.0, dtype=dtype)
    values.fill_diagonal_(16.0)
    t, grow = torch.arange(width), torch.ones(1)
    for ld in (width, width + 3):
        placed, lse, loss, out, _ = run_and_check(values, t, grow, ld)
        want = 16.0 + math.log1p((width - 1) * math.exp(-32.0))
        e = (width + 128) * U + 4 * U * want
        assert float((lse.double().cpu() - want).abs().max()) <= e
    # and with the target beside the diagonal: -1 there, +1 on the diagonal, 0 elsewhere
    placed, lse, loss, out, _ = run_and_check(values, (t + 1) % width, grow, width + 3)
    d = out.view.float().cpu()
    want = torch.eye(width) - torch.roll(torch.eye(width), 1, 1)
    assert float((d - want).abs().max()) <= 2.0**-7


def minus_infinity_rows(width, dtype):
    """the rows of the -inf cases at ``width`` and a target for each"""
    base, _, _ = draw(1, width, dtype, 77)
    rows, targets = [], []
    for k in (1, 8, 2048, 2049):
        if k < width:
            row = base[0].clone()
            row[:k] = -INF
            rows.append(row)
            targets.append(width - 1)
    for at in (0, width // 2, width - 1):
        row = torch.full((width, ), -INF, dtype=dtype)
        row[at] = base[0, at]
        rows += [row, row.clone()]
        targets += [at, (at + 1) % width]                   # its own place: loss 0; a -inf place: loss +inf, finite gradients
    for phase in (0, 1):
        row = base[0].clone()
        row[phase::2] = -INF
        rows.append(row)
        targets.append(1 - phase)
    return torch.stack(rows), torch.tensor(targets)


@pytest.mark.parametrize('width', (9, 2049, 4099))
@pytest.mark.parametrize('dtype', DTYPES)
def test_minus_infinity_has_probability_zero_and_gradient_plus_zero(dtype, width):
    values, t = minus_infinity_rows(width, dtype)
    g = torch.Generator().manual_seed(width)
    grow = torch.randn(values.shape[0], generator=g)                               # (both signs: -0 would show)
    for ld, offset in ((width, 1), (width + 3, 1), (width + 5, 0)):
        _, lse, loss, out, _ = run_and_check(values, t, grow, ld, offset=offset)
        assert not torch.isnan(lse).any() and not torch.isnan(out.view).any()
        single = (values != -INF).sum(1) == 1
        own = single & (values.gather(1, t[:, None])[:, 0] != -INF)
        assert not loss.cpu()[own].any() and bool((loss.cpu()[single & ~own] == INF).all())


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_row_of_minus_infinity_a_plus_infinity_and_a_nan_are_nan_rows_and_their_neighbours_are_untouched(dtype):
    for width in (9, 2049, 4099):
        for kind in range(4):
            values, t, grow = draw(3, width, dtype, 5 + kind)
            if kind == 0:
                values[1] = -INF
            elif kind == 1:
                values[1, width // 3] = INF
            elif kind == 2:
                values[1, width - 1] = float('nan')
            else:
                values[1] = -INF                            # a NaN among -inf only: no finite maximum to carry it
                values[1, width // 2] = float('nan')
            _, lse, loss, out, _ = run_and_check(values, t, grow, width + 3)
            assert torch.isnan(loss[1]) and torch.isnan(out.view[1]).all()
            assert torch.isfinite(loss[[0, 2]]).all() and torch.isfinite(out.view[[0, 2]]).all()
            assert (lse[1] == -INF) if kind == 0 else torch.isnan(lse[1])


@pytest.mark.parametrize('ignore_index', (-100, 3))
@pytest.mark.parametrize('dtype', DTYPES)
def test_ignored_rows_are_plus_zero(dtype, ignore_index):
    for width in (7, 257, 2049):
        values, t, grow = draw(5, width, dtype, 11)
        t[1] = t[4] = ignore_index
        t[0], t[2] = 3, width - 1                           # (3 is an ordinary class unless it is the ignored one)
        values[4, 0] = float('nan')                         # an ignored row is not read backward: +0 whatever it holds
        _, lse, loss, out, _ = run_and_check(values, t, grow, width + 3, ignore_index)
        ignored = (t == ignore_index).to(loss.device)
        assert int(ignored.sum()) >= 2
        assert not loss[ignored].any() and not torch.signbit(loss[ignored]).any()
        assert not out.view[ignored].any() and not torch.signbit(out.view[ignored]).any()
        assert torch.isfinite(lse[1]) and torch.isnan(lse[4])


@pytest.mark.parametrize('bad', ('width', -1, 2**40, -2**63))
@pytest.mark.parametrize('dtype', DTYPES)
def test_a_target_out_of_range_is_a_nan_row_and_nothing_else_is_touched(dtype, bad):
    for width in (9, 2049):
        values, t, grow = draw(3, width, dtype, 13)
        t[1] = width if bad == 'width' else bad
        placed, lse, loss, out, _ = run_and_check(values, t, grow, width + 3)          # (the other rows: within bound; the guard bands: unchanged)
        assert torch.isnan(loss[1]) and torch.isnan(out.view[1]).all() and torch.isfinite(lse).all()
        assert torch.isfinite(loss[[0, 2]]).all() and torch.isfinite(out.view[[0, 2]]).all()
        # in place as well: the guard band around the logits themselves
        cabi_x.cross_entropy_backward(placed.view, t.cuda(), lse, grow.cuda(), out=placed.view)
        assert placed.untouched() and torch.equal(bits(placed.view), bits(out.view))


@pytest.mark.parametrize('dtype', DTYPES)
def test_rows_of_equal_logits_sum_exactly(dtype):
    for c in (0.0, 2.5, 16.0, -16.0):
        for width in (1, 2, 9, 257, 2049, 4099):
            values = torch.full((3, width), c, dtype=dtype)
            t, grow = torch.tensor([0, width // 2, width - 1]), torch.tensor([1.0, -0.5, 3.0])
            _, lse, loss, out, _ = run_and_check(values, t, grow, width + 3)
            want = c + math.log(width)
            assert float((lse.double().cpu() - want).abs().max()) <= 4 * U * abs(want), (c, width)
            if width == 1:
                assert not loss.any() and not out.view.any()


@pytest.mark.parametrize('dtype', DTYPES)
def test_in_place_and_a_scalar_gradient_give_the_same_bits_and_calls_repeat(dtype):
    for rows, width, ld in ((1, 9, 9), (3, 257, 257), (5, 2049, 2052), (2, 4099, 4099)):
        values, t, grow = draw(rows, width, dtype, 21)
        t[0] = -100
        placed = Placed(values, ld)
        lse, loss, out = run(placed, t, grow)
        lse2, loss2, out2 = run(placed, t, grow)
        assert torch.equal(bits(lse), bits(lse2)) and torch.equal(bits(loss), bits(loss2)) and torch.equal(bits(out.view), bits(out2.view))
        scalar, vector = torch.tensor([0.375]), torch.full((rows, ), 0.375)
        _, _, by_scalar = run(placed, t, scalar)
        _, _, by_vector = run(placed, t, vector)
        assert torch.equal(bits(by_scalar.view), bits(by_vector.view))
        for g, want in ((grow, out), (scalar, by_scalar)):
            copy = Placed(values, ld)
            got = cabi_x.cross_entropy_backward(copy.view, t.cuda(), lse, g.cuda(), out=copy.view)
            assert got is copy.view and torch.equal(bits(copy.view), bits(want.view)) and copy.untouched()


def test_more_rows_than_workgroups_and_a_row_of_many_sweeps():
    # the cap on the workgroups, from the kernels' source: the binding's constant restates it, and the row count stands well beyond it
    source = (Path(__file__).resolve().parents[1] / 'fewbit_amd' / 'csrc' / 'fewbit_xent.hip').read_text()
    cap = int(re.search(r'constexpr size_t kMaxGroups = (\d+);', source).group(1))
    assert cabi_x.CROSS_ENTROPY_MAX_GROUPS == cap
    rows = 34 * cap + 369
    assert rows % cap and rows > 34 * cap
    for dtype in (torch.bfloat16, torch.float32):
        values, t, grow = draw(rows, 9, dtype, 31)
        t[::7] = -100
        run_and_check(values, t, grow)
        values, t, grow = draw(2, 131075, dtype, 33)
        run_and_check(values, t, grow, 131075 + 3)


def test_the_binding_refuses_what_the_kernels_do_not_take():
    x = torch.zeros(3, 8, device='cuda')
    t = torch.zeros(3, dtype=torch.int64, device='cuda')
    lse, _ = cabi_x.cross_entropy_forward(x, t)
    with pytest.raises(cabi_x.FewbitHipError):
        cabi_x.cross_entropy_forward(x.double(), t)
    with pytest.raises(cabi_x.FewbitHipError):
        cabi_x.cross_entropy_forward(x.t(), t[:8])
    with pytest.raises(cabi_x.FewbitHipError):
        cabi_x.cross_entropy_forward(x, t.int())
    with pytest.raises(cabi_x.FewbitHipError):
        cabi_x.cross_entropy_forward(x.cpu(), t.cpu())
    with pytest.raises(cabi_x.FewbitHipError):
        cabi_x.cross_entropy_backward(x, t, lse, torch.ones(2, device='cuda'))
    with pytest.raises(cabi_x.FewbitHipError, match='overlaps'):
        big = torch.zeros(4, 8, device='cuda')
        cabi_x.cross_entropy_backward(big[:3], t, lse, torch.ones(1, device='cuda'), out=big[1:])
