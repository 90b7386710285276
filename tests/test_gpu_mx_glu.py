"""``cabi_x.mx_glu_forward`` / ``mx_glu_backward`` on the GPU (include/fewbit_hipx.h, "The gate and the up as row blocks"; fewbit_amd/csrc/fewbit_mxglu.hip)
against what they are defined by: ``y`` is ``glu_forward``'s bit for bit, every cell buffer is ``mx_pack_host`` of its tensor with its seed bit for bit,
``d_gate`` and ``d_up`` hold the bounds ``tests/test_gpu_glu.py`` sets for the integer form (``check_gradients``, taken from there) against float64 on the
host decodes.  Shapes: one partial block, the block edge, a partial column tile with a partial last octet of columns, three blocks by four column
tiles; and once every tensor as a column block of ONE buffer whose rows are further apart than the width and which starts one element (2 bytes at
16 bits) off its 16-byte alignment: the element accesses and the ``[gate | up]`` halves.

The product cells: ``y^`` is never written, so it is obtained from the EXISTING product kernel -- ``glu_forward(g^, u^, keep=False)`` evaluates the same
expression ``round(act(g^) * u^)`` on the decodes, which every dtype here holds exactly -- and ``product_cells`` must be ``mx_pack_host`` of that, bit for
bit (the first of the two checks the issue offers, with the plain forward in place of an integer-form state, which cannot hold MX decodes)."""
import pytest
import torch

from fewbit_amd import cabi_x
from test_gpu_glu import check_gradients
from test_gpu_mx import DEV, DTYPES, defined, ids

pytestmark = pytest.mark.gpu
CASES = ((1, 8, False), (31, 64, False), (33, 72, False), (65, 200, False), (33, 72, True))     # rows, width, strided
SEEDS = (0x1234567, 0x89abcdef01, 0xfeed5, 0xbeef77, 0xc0ffee)                              # gate, up, d_gate, d_up, product
every = pytest.mark.parametrize('dtype, format, activation', [(d, f, a) for d in DTYPES for f in ('fp4', 'fp6') for a in ('silu', 'gelu')], ids=ids)


def blocks(rows, width, dtype, strided, count, values=()):
    """`count` rows x width tensors on the device holding `values` (7 where there are none): dense, or the column blocks of ONE buffer with rows
    count * width + 3 apart that starts one element off its 16-byte alignment -> (the tensors, the gaps of that buffer)"""
    if not strided:
        return [v.to(DEV) for v in values] + [torch.full((rows, width), 7.0, dtype=dtype, device=DEV) for _ in range(count - len(values))], None
    ld = count * width + 3
    whole = torch.full((rows * ld + 1, ), 7.0, dtype=dtype, device=DEV)[1:].view(rows, ld)
    parts = [whole[:, i * width:(i + 1) * width] for i in range(count)]
    for part, v in zip(parts, values):
        part.copy_(v)
    return parts, whole[:, count * width:]


def problem(rows, width, dtype, strided):
    gen = torch.Generator().manual_seed(1000 * rows + width)
    host = [(3 * torch.randn(rows, width, generator=gen)).to(dtype) for _ in range(3)]
    (gate, up), _ = blocks(rows, width, dtype, strided, 2, host[:2])
    return host, gate, up


def raw(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def parts_of(state, rows, width, format):
    half, need = state.numel() // 2, cabi_x.mx_bytes(rows, width, format)
    assert state.numel() == cabi_x.mx_glu_state_bytes(rows, width, format) and half % 16 == 0
    return state[:need].cpu(), state[half:half + need].cpu()


@every
def test_forward_is_glu_forward_and_two_mx_packs(dtype, format, activation):
    for rows, width, strided in CASES:
        (g, u, _), gate, up = problem(rows, width, dtype, strided)
        (out, ), gaps = blocks(rows, width, dtype, strided, 1)
        y, state = cabi_x.mx_glu_forward(gate, up, activation, format, SEEDS[:2], y=out)
        assert torch.equal(raw(y), raw(cabi_x.glu_forward(gate, up, activation, keep=False)[0])) and (gaps is None or bool((gaps == 7).all())), (rows, width)
        for part, values, seed in zip(parts_of(state, rows, width, format), (g, u), SEEDS):
            assert torch.equal(defined(part, rows, width), defined(cabi_x.mx_pack_host(values.float(), seed, format, 'kept'), rows, width)), (rows, width)
        # the seeds as words on the device: the same bytes; gate == up: two independent roundings
        words = torch.tensor(SEEDS[:2], dtype=torch.int64, device=DEV)
        by_words = parts_of(cabi_x.mx_glu_forward(gate, up, activation, format, words)[1], rows, width, format)
        assert all(torch.equal(defined(a, rows, width), defined(b, rows, width)) for a, b in zip(by_words, parts_of(state, rows, width, format)))
        first, second = parts_of(cabi_x.mx_glu_forward(gate, gate, activation, format, SEEDS[:2])[1], rows, width, format)
        assert rows * width < 64 or not torch.equal(defined(first, rows, width), defined(second, rows, width))
    with pytest.raises(cabi_x.FewbitHipError):
        cabi_x.mx_glu_forward(gate, up, activation, format, (5, 5))


@every
def test_backward_is_the_formulas_on_the_decodes_and_three_mx_packs(dtype, format, activation):
    for rows, width, strided in CASES:
        (g, u, gy_host), gate, up = problem(rows, width, dtype, strided)
        state = cabi_x.mx_glu_forward(gate, up, activation, format, SEEDS[:2])[1]
        g_hat, u_hat = (cabi_x.mx_unpack_host(part, rows, width, format) for part in parts_of(state, rows, width, format))
        (gy, d_gate, d_up), gaps = blocks(rows, width, dtype, strided, 3, (gy_host, ))
        outs = cabi_x.mx_glu_backward(gy, state, activation, format, SEEDS[2:], d_gate=d_gate, d_up=d_up)
        assert outs[0] is d_gate and outs[1] is d_up and (gaps is None or bool((gaps == 7).all()))
        check_gradients(d_gate.cpu(), d_up.cpu(), gy_host, g_hat, u_hat, activation, dtype, f'{rows}x{width} {format}')
        product = cabi_x.glu_forward(g_hat.to(dtype).to(DEV), u_hat.to(dtype).to(DEV), activation, keep=False)[0]
        assert torch.equal(g_hat.to(dtype).float(), g_hat) and torch.equal(u_hat.to(dtype).float(), u_hat)       # (the decodes are exact in dtype)
        for cells, tensor, seed, fmt, role in zip(outs[2:], (d_gate, d_up, product), SEEDS[2:], ('fp8', 'fp8', format), ('grad', 'grad', 'kept')):
            want = cabi_x.mx_pack_host(tensor.float().cpu(), seed, fmt, role)
            assert torch.equal(defined(cells.cpu(), rows, width), defined(want, rows, width)), (rows, width, fmt, role)
        # the seeds as words on the device, and outputs that are not wanted
        words = torch.tensor(SEEDS[2:], dtype=torch.int64, device=DEV)
        again = cabi_x.mx_glu_backward(gy, state, activation, format, words, want=(False, True, True, False, True))
        assert again[0] is None and again[3] is None and torch.equal(raw(again[1]), raw(d_up))
        assert all(torch.equal(defined(again[i], rows, width), defined(outs[i], rows, width)) for i in (2, 4))


@pytest.mark.parametrize('format', ('fp4', 'fp6'))
def test_a_poisoned_state_cell_is_nan_on_its_rows_of_its_column_and_nowhere_else(format):
    rows, width = 65, 72
    _, gate, up = problem(rows, width, torch.bfloat16, False)
    gy = torch.ones(rows, width, dtype=torch.bfloat16, device=DEV)
    state = cabi_x.mx_glu_forward(gate, up, 'silu', format, SEEDS[:2])[1]
    clean = cabi_x.mx_glu_backward(gy, state, 'silu', format, SEEDS[2:])
    state[state.numel() // 2 + 1 * width + 7] = 0xFF                       # the scale byte of block 1, column 7 of up
    got = cabi_x.mx_glu_backward(gy, state, 'silu', format, SEEDS[2:])
    nan = torch.zeros(rows, width, dtype=torch.bool, device=DEV)
    nan[32:64, 7] = True
    for a, b in zip(got[:2], clean[:2]):
        assert torch.equal(a.isnan(), nan) and torch.equal(a[~nan], b[~nan])
    for a in got[2:]:
        assert int((a[:3 * width] == 0xFF).sum()) == 1 and a[width + 7] == 0xFF    # the cells written from them: poisoned by the rule of the pack
