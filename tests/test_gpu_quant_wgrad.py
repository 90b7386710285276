"""``cabi_x.quant_wgrad`` on the GPU (include/fewbit_hipx.h, "The weight gradient from the packed form"; fewbit_amd/csrc/fewbit_qgemm.hip) against the
float64 product of the same operands built on the HOST: the packed bytes by ``quant_pack_host``, their fp32 decode by ``quant_unpack_host``, ``op`` as
the header defines it (rounded once to the gradient's dtype; head + tail for bf16 at 8 bits).  Bound, entry by entry:
``2 (rows + slices + 2) 2^-24 (|G|^T |op|)`` -- products of 16-bit operands are exact in fp32, every addition of the accumulation and of the slice
sum errs by at most one fp32 ulp of a partial sum that ``sum |g| |x^|`` bounds (one ulp, not half: the matrix pipe's additions are not documented as
round-to-nearest); a misplaced element, row or group is off by order 1."""
import pytest
import torch

from fewbit_amd import cabi_x

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BM, BN, BK = cabi_x.QUANT_WGRAD_TILE
SLICED = next(rows for rows in range(2 * BK, 64 * BK) if cabi_x.quant_wgrad_slices(rows, 64, 8) >= 2) + 3
# rows x in x out: a K tail inside a block of eight, a whole stage, ragged stages, the slice sum; then the tile edges
SHAPES = [(rows, 64, 8) for rows in (1, 7, BK - 1, BK, BK + 9, 2 * BK + 8 * 3 + 5, SLICED)] + [(BK + 9, BN + 64, BM - 8), (BK + 9, BN + 64, BM + 8), (SLICED, 64, BM + 8)]
ids = lambda v: str(v).split('.')[-1] if isinstance(v, torch.dtype) else 'x'.join(map(str, v)) if isinstance(v, tuple) else None


def problem(shape, dtype, bits, poison=False):
    """-> (G with BK rows of NaN behind it, the packed buffer with 0xFF bytes behind it, the float64 product, its bound)"""
    rows, fin, fout = shape
    gen = torch.Generator().manual_seed(rows + 3 * fin + 7 * fout + bits)
    g = torch.randn(rows, fout, generator=gen).to(dtype)
    x = (torch.randn(rows, fin, generator=gen) * (1 + torch.arange(fin) % 5)).to(dtype)
    if poison:
        x[rows // 2, fin - 7] = float('inf')
    packed = cabi_x.quant_pack_host(x.float(), 20260 + bits, bits)
    decoded = cabi_x.quant_unpack_host(packed, rows * fin, bits).view(rows, fin)
    head = decoded.to(dtype)
    op = head.double()
    if bits == 8 and dtype == torch.bfloat16:
        op = op + (decoded - head.float()).to(dtype).double()
    slices = cabi_x.quant_wgrad_slices(rows, fin, fout)
    bound = 2 * (rows + slices + 2) * 2.0**-24 * (g.double().abs().T @ op.abs())
    behind = torch.full((rows + BK, fout), float('nan'), dtype=dtype, device=DEV)
    behind[:rows] = g.to(DEV)
    buffer = torch.full((packed.numel() + 64, ), 0xFF, dtype=torch.uint8, device=DEV)
    buffer[:packed.numel()] = packed.to(DEV)
    return behind[:rows], buffer[:packed.numel()], g.double().T @ op, bound


def guarded(count, dtype, fill):
    """a buffer of ``count`` elements with 16 guard elements behind it"""
    whole = torch.full((count + 16, ), fill, dtype=dtype, device=DEV)
    return whole, whole[:count]


def run(shape, dtype, bits, g, packed, out_dtype=torch.float32):
    """one call with guard words behind ``out`` and the workspace, both checked"""
    rows, fin, fout = shape
    need = cabi_x.quant_wgrad_workspace(dtype, rows, fin, fout, bits)
    assert (need > 0) == (cabi_x.quant_wgrad_slices(rows, fin, fout) > 1) and need <= rows * fin * 2
    whole, out = guarded(fout * fin, out_dtype, -7.0)
    scratch, workspace = guarded(need, torch.uint8, 0xA5)
    got = cabi_x.quant_wgrad(g, packed, fin, bits, out_dtype, out.view(fout, fin), workspace=workspace if need else None)
    torch.cuda.synchronize()
    assert bool((whole[fout * fin:] == -7.0).all()) and bool((scratch[need:] == 0xA5).all())
    return got.clone()


@pytest.mark.parametrize('bits', cabi_x.QUANT_BITS)
@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float16), ids=ids)
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_the_product_against_float64_of_the_same_operands(shape, dtype, bits):
    g, packed, want, bound = problem(shape, dtype, bits)
    got = run(shape, dtype, bits, g, packed)
    err = (got.cpu().double() - want).abs()
    print(f'{shape} {dtype} bits {bits}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}')
    assert bool((err <= bound).all())
    # a 16-bit result is that fp32 result rounded once; the same call again gives the same bits
    assert torch.equal(run(shape, dtype, bits, g, packed, dtype).view(torch.int16), got.to(dtype).view(torch.int16))
    assert torch.equal(run(shape, dtype, bits, g, packed), got)


@pytest.mark.parametrize('bits', cabi_x.QUANT_BITS)
@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float16), ids=ids)
def test_one_poisoned_group_is_nan_on_its_64_columns_and_nowhere_else(dtype, bits):
    shape = (SLICED, BN + 64, 16)
    g, packed, want, bound = problem(shape, dtype, bits, poison=True)
    got = run(shape, dtype, bits, g, packed).cpu().double()
    nan = torch.zeros(shape[2], shape[1], dtype=torch.bool)
    nan[:, BN:] = True                                                   # the group of feature in - 7: the last 64 columns, in every row
    assert torch.equal(got.isnan(), nan) and torch.equal(want.isnan(), nan)
    assert bool(((got - want).abs()[~nan] <= bound[~nan]).all())


@pytest.mark.parametrize('shape', ((BK + 9, BN + 64, BM + 8), (SLICED, 64, 8)), ids=ids)
def test_a_captured_call_replays_the_eager_result(shape):
    g, packed, want, bound = problem(shape, torch.bfloat16, 8)
    eager = cabi_x.quant_wgrad(g, packed, shape[1], 8, torch.float32)
    out = torch.zeros_like(eager)
    need = cabi_x.quant_wgrad_workspace(torch.bfloat16, *shape, 8)
    workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cabi_x.quant_wgrad(g, packed, shape[1], 8, torch.float32, out, workspace=workspace)
    for _ in range(3):
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
