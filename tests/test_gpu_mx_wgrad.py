"""``cabi_x.mx_wgrad`` on the GPU (include/fewbit_hipx.h, "The row blocks of a seed"; fewbit_amd/csrc/fewbit_mx.hip) against the float64 product of the
operands decoded on the HOST (``mx_pack_host`` / ``mx_unpack_host``).  The bound is NOT that of tests/test_gpu_quant_wgrad.py: the scaled instruction does
not add its 64 products in fp32.  Measured with 2^10 + 2^-a in one K step: it aligns the products of a step to the largest and keeps what lies at or
above 2^-13 of that one's binade, cutting the rest off towards zero (a product of 2^-3 beside 2^10 arrives whole, 2^-4 is gone).  So, entry by entry:
``sum over K steps of 64 * 2^-13 * max|g^| * max|x^|`` (the maxima over the step's 64 rows: each product loses less than one such unit, whether the
hardware aligns to the largest product or to the largest exponents) ``+ 2 (steps + slices + 2) 2^-24 (|G^|^T |X^|)`` (one fp32 ulp for each addition
of a step's sum to the accumulator and of the slice sum).  With the fp32 bound ``2 (rows + slices + 2) 2^-24 (|G^|^T |X^|)`` the worst entries were
1.4 - 4.1 times over at 31 .. 65 rows and 0.2 - 0.7 of it at 131 and 165 rows.  A misplaced element, nibble order, row block or scale is off by order 1,
a hundred times this bound.  Both operands are packed on the host, so that the reference shares nothing with the GPU; the last test packs G on the
GPU from a store with NaN rows behind it, holds it to the host's bytes and multiplies that buffer, one of its cells poisoned."""
import pytest
import torch

from fewbit_amd import cabi_x

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BM, BN, BK = cabi_x.MX_WGRAD_TILE
SLICED = next(rows for rows in range(BK, 64 * BK) if cabi_x.mx_wgrad_slices(rows, 32, 32) >= 2) + 3
# rows x in x out: inside a block, a whole block, a half step, a whole step, ragged steps, the slice sum; then the tile edges
SHAPES = [(rows, 32, 32) for rows in (1, 31, 32, 33, 63, 64, 65, 2 * 64 + 32 + 5, SLICED)] + [(65, BN - 32, BM + 32), (65, BN + 32, BM - 32), (SLICED, BN + 32, BM + 32)]
ids = lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else None


def problem(shape, format, poison=False, g=None):
    """-> (the fp8 buffer of G and the `format` buffer of X, each with 0xFF bytes behind it, the float64 product of their decodes, its bound)"""
    rows, fin, fout = shape
    gen = torch.Generator().manual_seed(rows + 3 * fin + 7 * fout)
    g = torch.randn(rows, fout, generator=gen) * (1 + torch.arange(fout) % 3) if g is None else g
    x = torch.randn(rows, fin, generator=gen) * (1 + torch.arange(fin) % 5)
    if poison:
        x[rows // 2, fin - 7] = float('inf')
    buffers, decoded = [], []
    for values, fmt, role in ((g, 'fp8', 'grad'), (x, format, 'kept')):
        packed = cabi_x.mx_pack_host(values, 20260, fmt, role)
        decoded.append(cabi_x.mx_unpack_host(packed, *values.shape, fmt).double())
        behind = torch.full((packed.numel() + 4096, ), 0xFF, dtype=torch.uint8, device=DEV)
        behind[:packed.numel()] = packed.to(DEV)
        buffers.append(behind[:packed.numel()])
    steps = -(-rows // BK)
    top = [torch.cat((d.abs(), torch.zeros(steps * BK - rows, d.shape[1], dtype=d.dtype))).nan_to_num(nan=0.0).view(steps, BK, -1).amax(dim=1) for d in decoded]
    bound = 64 * 2.0**-13 * (top[0].T @ top[1]) + 2 * (steps + cabi_x.mx_wgrad_slices(rows, fin, fout) + 2) * 2.0**-24 * (decoded[0].abs().T @ decoded[1].abs())
    return buffers[0], buffers[1], decoded[0].T @ decoded[1], bound


def run(shape, format, g, x, out_dtype=torch.float32):
    """one call with guard words behind ``out`` and the workspace, both checked"""
    rows, fin, fout = shape
    need = cabi_x.mx_wgrad_workspace(rows, fin, fout, format)
    assert (need > 0) == (cabi_x.mx_wgrad_slices(rows, fin, fout) > 1) and need <= rows * fin * 2
    whole = torch.full((fout * fin + 16, ), -7.0, dtype=out_dtype, device=DEV)
    scratch = torch.full((need + 16, ), 0xA5, dtype=torch.uint8, device=DEV)
    got = cabi_x.mx_wgrad(g, x, rows, fin, fout, format, out_dtype, whole[:fout * fin].view(fout, fin), workspace=scratch[:need] if need else None)
    torch.cuda.synchronize()
    assert bool((whole[fout * fin:] == -7.0).all()) and bool((scratch[need:] == 0xA5).all())
    return got.clone()


@pytest.mark.parametrize('format', ('fp4', 'fp6'))
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_the_product_against_float64_of_the_same_operands(shape, format):
    g, x, want, bound = problem(shape, format)
    got = run(shape, format, g, x)
    err = (got.cpu().double() - want).abs()
    print(f'{shape} {format}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}')
    assert bool((err <= bound).all())
    # a 16-bit result is that fp32 result rounded once; the same call again gives the same bits
    for dtype in (torch.bfloat16, torch.float16):
        assert torch.equal(run(shape, format, g, x, dtype).view(torch.int16), got.to(dtype).view(torch.int16))
    assert torch.equal(run(shape, format, g, x), got)


@pytest.mark.parametrize('format', ('fp4', 'fp6'))
def test_one_poisoned_cell_is_nan_on_exactly_its_column(format):
    shape = (SLICED, BN + 32, 64)
    g, x, want, bound = problem(shape, format, poison=True)
    got = run(shape, format, g, x).cpu().double()
    nan = torch.zeros(shape[2], shape[1], dtype=torch.bool)
    nan[:, shape[1] - 7] = True
    assert torch.equal(got.isnan(), nan) and torch.equal(want.isnan(), nan)
    assert bool(((got - want).abs()[~nan] <= bound[~nan]).all())


@pytest.mark.parametrize('shape', ((65, BN + 32, BM + 32), (SLICED, 32, 32)), ids=ids)
def test_a_captured_call_replays_the_eager_result(shape):
    g, x, want, bound = problem(shape, 'fp4')
    eager = cabi_x.mx_wgrad(g, x, *shape, 'fp4')
    out = torch.zeros_like(eager)
    workspace = torch.empty(max(cabi_x.mx_wgrad_workspace(*shape, 'fp4'), 16), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cabi_x.mx_wgrad(g, x, *shape, 'fp4', torch.float32, out, workspace=workspace)
    for _ in range(3):
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_g_packed_on_the_gpu_from_a_nan_backed_store_with_one_poisoned_cell_is_nan_on_exactly_its_row():
    shape = rows, fin, fout = (SLICED, 32, 64)
    g = torch.randn(rows, fout, generator=torch.Generator().manual_seed(8)).bfloat16()
    g[rows - 2, 3] = float('nan')
    host, x, want, bound = problem(shape, 'fp6', g=g.float())
    store = torch.full((rows + BK, fout), float('nan'), dtype=torch.bfloat16, device=DEV)
    store[:rows] = g.to(DEV)
    packed, scales = cabi_x.mx_pack(store[:rows], 20260, 'fp8', 'grad'), -(-rows // 32) * fout
    assert torch.equal(packed[:scales], host[:scales]) and torch.equal(packed[-(-scales // 16) * 16:], host[-(-scales // 16) * 16:])
    got = run(shape, 'fp6', packed, x).cpu().double()
    nan = torch.zeros(fout, fin, dtype=torch.bool)
    nan[3] = True
    assert torch.equal(got.isnan(), nan) and torch.equal(want.isnan(), nan) and bool(((got - want).abs()[~nan] <= bound[~nan]).all())
