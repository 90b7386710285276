"""The step of a chunked LM head on the GPU (include/fewbit_hipx.h, fewbit_hipx_cross_entropy_step; fewbit_amd/csrc/fewbit_xent.hip, step_kernel), at the
binding level: lse, loss and the gradient written over the logits against the float64 host evaluation within the derived bounds of the header
(tests/xent_harness.py), on rows that start on no 16-byte boundary, at both sides of every tier of the staging capacity and beyond the last."""
import pytest
import torch

from fewbit_amd import cabi_x
from xent_harness import DTYPES, Placed, bits, check, draw

pytestmark = pytest.mark.gpu

INF = float('inf')
STAGED = cabi_x.CROSS_ENTROPY_STEP_STAGED_BYTES
WIDTHS = (1, 7, 8, 9, 63, 65, 255, 257, 2047, 2049, 4099)


def reread(dtype):
    """a width that no tier holds: the row is read twice, by the pair's two launches"""
    return STAGED[-1] // dtype.itemsize + 5


def edges(dtype):
    """the last width of every tier, the one below and the first of the next"""
    return tuple(b // dtype.itemsize + d for b in STAGED for d in (-1, 0, 1))


def run_and_check(values, t, grow, ld=None, ignore_index=-100):
    placed = Placed(values, ld)
    lse, loss = cabi_x.cross_entropy_step(placed.view, t.cuda(), grow.cuda(), ignore_index)
    worst = check(values, t, grow, lse, loss, placed.view, ignore_index)
    assert placed.untouched(), 'something outside the rows was written'
    return placed, lse, loss, worst


@pytest.mark.parametrize('width', WIDTHS + ('edges', ))
@pytest.mark.parametrize('dtype', DTYPES)
def test_every_lse_loss_and_gradient_is_inside_its_bound(dtype, width):
    for width in edges(dtype) if width == 'edges' else (width, ):
        worst = [0.0, 0.0, 0.0]
        for rows in (1, 3, 5):
            values, t, grow = draw(rows, width, dtype, rows)
            for ld, g in ((width, grow), (width, grow[:1]), (width + 3, grow), (width + 3, grow[:1])):
                worst = [max(a, b) for a, b in zip(worst, run_and_check(values, t, g, ld)[3])]
        print(f'{dtype} width {width}: worst fractions of the bounds (lse, loss, dlogits) = {worst[0]:.3f}, {worst[1]:.3f}, {worst[2]:.3f}')


@pytest.mark.parametrize('width', (9, 2049, 'reread'))
@pytest.mark.parametrize('dtype', DTYPES)
def test_minus_infinity_has_probability_zero_and_gradient_plus_zero(dtype, width):
    width = reread(dtype) if width == 'reread' else width
    base, _, _ = draw(1, width, dtype, 77)
    rows, targets = [], []
    for k in (1, 8, 2048):
        if k < width:
            rows.append(base[0].clone())
            rows[-1][:k] = -INF
            targets.append(width - 1)
    for at in (0, width // 2, width - 1):
        row = torch.full((width, ), -INF, dtype=dtype)
        row[at] = base[0, at]
        rows += [row, row.clone()]
        targets += [at, (at + 1) % width]                   # its own place: loss 0; a -inf place: loss +inf, finite gradients
    rows.append(base[0].clone())
    rows[-1][1::2] = -INF
    targets.append(0)
    values, t = torch.stack(rows), torch.tensor(targets)
    grow = torch.randn(len(rows), generator=torch.Generator().manual_seed(width))           # (both signs: -0 would show)
    placed, lse, loss, _ = run_and_check(values, t, grow, width + 3)
    assert not torch.isnan(lse).any() and not torch.isnan(placed.view).any()


@pytest.mark.parametrize('kind', range(4))
@pytest.mark.parametrize('dtype', DTYPES)
def test_a_row_of_minus_infinity_a_plus_infinity_and_a_nan_are_nan_rows_and_their_neighbours_are_untouched(dtype, kind):
    for width in (9, 2049, reread(dtype)):
        values, t, grow = draw(3, width, dtype, 5 + kind)
        if kind == 0:
            values[1] = -INF
        elif kind == 1:
            values[1, width // 3] = INF
        elif kind == 2:
            values[1, width - 1] = float('nan')
        else:
            values[1] = -INF                                # a NaN among -inf only: no finite maximum to carry it
            values[1, width // 2] = float('nan')
        placed, lse, loss, _ = run_and_check(values, t, grow, width + 3)
        assert torch.isnan(loss[1]) and torch.isnan(placed.view[1]).all()
        assert torch.isfinite(loss[[0, 2]]).all() and torch.isfinite(placed.view[[0, 2]]).all()
        assert (lse[1] == -INF) if kind == 0 else torch.isnan(lse[1])


@pytest.mark.parametrize('ignore_index', (-100, 3))
@pytest.mark.parametrize('dtype', DTYPES)
def test_ignored_rows_are_plus_zero_and_still_have_their_lse(dtype, ignore_index):
    for width in (9, 2049, reread(dtype)):
        values, t, grow = draw(5, width, dtype, 11)
        t[1] = t[4] = ignore_index
        t[0], t[2] = 3, width - 1                           # (3 is an ordinary class unless it is the ignored one)
        values[4, 0] = float('nan')                         # +0 whatever the row holds
        placed, lse, loss, _ = run_and_check(values, t, grow, width + 3, ignore_index)
        ignored = (t == ignore_index).cuda()
        assert int(ignored.sum()) >= 2
        assert not loss[ignored].any() and not torch.signbit(loss[ignored]).any()
        assert not placed.view[ignored].any() and not torch.signbit(placed.view[ignored]).any()
        assert torch.isfinite(lse[1]) and torch.isnan(lse[4])


@pytest.mark.parametrize('bad', ('width', -1, 2**40, -2**63))
@pytest.mark.parametrize('dtype', DTYPES)
def test_a_target_out_of_range_is_a_nan_row_and_nothing_else_is_touched(dtype, bad):
    for width in (9, 2049, reread(dtype)):
        values, t, grow = draw(3, width, dtype, 13)
        t[1] = width if bad == 'width' else bad
        placed, lse, loss, _ = run_and_check(values, t, grow, width + 3)
        assert torch.isnan(loss[1]) and torch.isnan(placed.view[1]).all() and torch.isfinite(lse).all()
        assert torch.isfinite(loss[[0, 2]]).all() and torch.isfinite(placed.view[[0, 2]]).all()


@pytest.mark.parametrize('dtype, rows, width', ((torch.bfloat16, 34 * cabi_x.CROSS_ENTROPY_MAX_GROUPS + 369, 9), (torch.float32, 3 * cabi_x.CROSS_ENTROPY_MAX_GROUPS + 5, 9),
                                                (torch.float32, 261, reread(torch.float32))))
def test_more_rows_than_workgroups_of_either_variant(dtype, rows, width):
    values, t, grow = draw(rows, width, dtype, 31)
    t[::7] = -100
    run_and_check(values, t, grow)


@pytest.mark.parametrize('dtype', DTYPES)
def test_calls_repeat_to_the_bit_and_give_the_bits_of_the_pair_where_the_walk_is_the_pairs(dtype):
    for rows, width, gap in ((1, 9, 0), (5, 2049, 3), (3, STAGED[0] // dtype.itemsize + 1, 0), (2, reread(dtype), 1)):
        values, t, grow = draw(rows, width, dtype, 21)
        t[0], ld = -100, width + gap
        first, again = Placed(values, ld), Placed(values, ld)
        lse, loss = cabi_x.cross_entropy_step(first.view, t.cuda(), grow.cuda())
        lse2, loss2 = cabi_x.cross_entropy_step(again.view, t.cuda(), grow.cuda())
        assert torch.equal(bits(lse), bits(lse2)) and torch.equal(bits(loss), bits(loss2)) and torch.equal(bits(first.view), bits(again.view))
        if width * dtype.itemsize <= STAGED[0] or width * dtype.itemsize > STAGED[-1]:
            # the first tier walks a row as the forward / backward pair does (256 lanes, the same merge), and beyond the last the pair runs: the same bits
            pair = Placed(values, ld)
            lse3, loss3 = cabi_x.cross_entropy_forward(pair.view, t.cuda())
            cabi_x.cross_entropy_backward(pair.view, t.cuda(), lse3, grow.cuda(), out=pair.view)
            assert torch.equal(bits(lse), bits(lse3)) and torch.equal(bits(loss), bits(loss3)) and torch.equal(bits(first.view), bits(pair.view))

