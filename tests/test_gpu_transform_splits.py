"""Both sampled-transform kernel pairs at EVERY row count of their dispatch table, in every dtype and through every entry point.

Each of the 38 row counts has its own split N = N1 x N2 and with it its own template instantiations of both passes: per input dtype,
output dtype, row source (an explicit idx, the rows of a seed) and plain or zero-extended pass A.  The digit maps, the twiddle tables,
the sort of the seeded rows and the partner index of the DFT's pass B are per-N code, so a fault at one N shows at that N only.  This
file enumerates the table and leaves no cell out:

    1  the table is the 38 counts written out below, in both libraries
    2  every k once (p = rows, a permutation: a wrong digit map cannot hide behind the sample), fp32, against the float64 transform
    3  every input / output dtype on ~500 sampled rows and the corners, against the float64 transform
    4  the rows of a seed == the explicit call on cabi.sampled_rows(seed), bit for bit, the seed by value and as a device word
    5  the zero-extended pairs == the plain entry points on a zero-filled copy, bit for bit, NaN behind everything they may not read
    6  the zero-extended pass A where its 32-bit buffer offsets have the top bit set (2 GiB and more), and at the exact limit of its span

Sections 2 and 3 use the bound of DESIGN section 6 that every transform test uses (helpers.sampled_rows_check, shown to have teeth in
tests/test_transform_splits_host.py):

    fp32 result              |err| <= 3e-6 max|y|
    bf16 / fp16 result       |err| <= 2^-8 |y| / 2^-11 |y| + 3e-6 max|y|       (one rounding of the fp32 result to the 16-bit dtype)

against `np.fft.fft(x, axis=0, norm='ortho')[idx] * scale` ('dft') and `fewbit.fft.dct(x.double(), dim=0, norm='ortho')[idx] * scale`
('dct'; tests/test_linear.py pins it to scipy), float64 on the host.  The inputs are multiples of 1/16 below 4 in magnitude: exact in
all three dtypes, so one float64 reference serves every dtype, and a fp32 result from 16-bit input gets the fp32 bound.  Sections 4 to 6
are bit-equalities with no tolerance.

Shapes: 66 features behind a leading dimension of 70 (one full 64-feature tile and an edge tile) up to 32768 rows, 7 features behind
a leading dimension of 11 above (an odd count: the last complex column has no partner).  Sections 2 to 4 of one (kind, rows) share one
input and one float64 transform (the module-scoped fixture `cell`)."""
import numpy as np
import pytest
import torch

import fewbit
from fewbit_amd import cabi, cabi_x, linear
from helpers import ROUNDING, sampled_rows_check

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
KINDS = ('dct', 'dft')
# the dispatch table of fewbit_fft4.h (split_rows), written out: a row count added there fails test_the_table_is_complete until it is added here
ROWS = (256, 512, 768, 1024, 1280, 1536, 2048, 2304, 2560, 3072, 3584, 3840, 4096, 4608, 5120, 6144, 7168, 7680, 8192, 9216, 10240, 12288,
        14336, 15360, 16384, 18432, 20480, 24576, 28672, 30720, 32768, 36864, 40960, 49152, 57344, 65536, 131072, 262144)
CELLS = [(kind, rows) for kind in KINDS for rows in ROWS]
SCALE = 0.75
SEEDS = (0x9e3779b97f4a7c15, 0x1234567890abcdef)           # the first has its top bit set


@pytest.fixture(autouse=True)
def _native():
    prev = linear.use_native_sketch(True)
    yield
    linear.use_native_sketch(prev)


def _cell_id(cell):
    return f'{cell[0]}-{cell[1]}'


def _integers(rows, width, seed):
    """multiples of 1/16 below 4 in magnitude: exact in all three dtypes (the data of tests/test_gpu_dft.py)"""
    return torch.randint(-64, 64, (rows, width), generator=torch.Generator().manual_seed(seed)).double() / 16.0


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _plain(kind, m, idx, scale, out_dtype=None):
    if kind == 'dct':
        return cabi.sampled_dct(m, idx, scale)
    return cabi_x.sampled_dft(m, idx, scale, out_dtype=out_dtype)


def _seeded(kind, m, p, seed, scale):
    return cabi.sampled_dct_seeded(m, p, seed, scale) if kind == 'dct' else cabi_x.sampled_dft_seeded(m, p, seed, scale)


def _zext(kind, x, rows, idx, scale):
    return cabi_x.sampled_dct_zext(x, rows, idx, scale) if kind == 'dct' else cabi_x.sampled_dft_zext(x, rows, idx, scale)


def _zext_seeded(kind, x, rows, p, seed, scale):
    return cabi_x.sampled_dct_zext_seeded(x, rows, p, seed, scale) if kind == 'dct' else cabi_x.sampled_dft_zext_seeded(x, rows, p, seed, scale)


def _word(seed):
    """the seed as the int64 device word the kernel reads when it runs"""
    return torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed], dtype=torch.int64, device=DEV)


class Cell:
    """one (kind, rows): the host input behind its leading dimension and its float64 transform, computed once and left unchanged"""

    def __init__(self, kind, rows):
        self.kind, self.rows = kind, rows
        self.features = 66 if rows <= 32768 else 7
        self.ld = self.features + 4
        self.wide = _integers(rows, self.ld, rows + (kind == 'dft'))
        data = self.wide[:, :self.features]
        if kind == 'dft':
            self.full = torch.from_numpy(np.fft.fft(data.numpy(), axis=0, norm='ortho'))
        else:
            self.full = fewbit.fft.dct(data, dim=0, norm='ortho')

    def x(self, dtype):
        """the device view of `dtype`: rows x features, unit stride along the features, the leading dimension 4 larger"""
        view = self.wide.to(dtype).to(DEV)[:, :self.features]
        assert view.stride(0) == self.ld and not view.is_contiguous()
        return view

    def want(self, idx):
        return self.full[idx] * SCALE


@pytest.fixture(scope='module', params=CELLS, ids=_cell_id)
def cell(request):
    return Cell(*request.param)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_table_is_complete():
    """the candidates odd x 2^k in [256, 262144], odd in 1, 3, 5, 7, 9, 15, for which the DCT's library has a kernel are exactly ROWS (38);
    the DFT's library agrees at every candidate, and each count is its own ceiling"""
    candidates = sorted({odd << k for odd in (1, 3, 5, 7, 9, 15) for k in range(19) if 256 <= odd << k <= 262144})
    have = [rows for rows in candidates if cabi.sampled_dct_workspace_bytes(rows, 1, 1) != 0]
    assert len(have) == 38 and tuple(have) == ROWS, have
    assert [rows for rows in candidates if cabi_x.sampled_dft_workspace_bytes(rows, 1, 1) != 0] == have
    for rows in have:
        assert cabi_x.sampled_rows_ceil(rows) == rows
        for dtype in DTYPES:
            assert cabi.sampled_dct_workspace_bytes(rows, 1, 1, dtype) == cabi_x.sampled_dft_workspace_bytes(rows, 1, 1, dtype) != 0
    assert len(CELLS) == 76 and len(set(CELLS)) == 76


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_every_k_once_in_fp32_is_the_float64_transform(cell):
    """p = rows, idx a seeded permutation, scale 0.75: |err| <= 3e-6 max|y| at every k; 'dft': the imaginary plane is exactly 0 at k = 0
    and k = rows / 2"""
    kind, rows = cell.kind, cell.rows
    idx = torch.randperm(rows, generator=torch.Generator().manual_seed(rows))
    got = _plain(kind, cell.x(torch.float32), idx.to(DEV), SCALE)
    assert got.dtype == torch.float32 and got.shape == ((2, ) if kind == 'dft' else ()) + (rows, cell.features) and got.is_contiguous()
    ok, worst = sampled_rows_check(got, cell.want(idx))
    print(f'\nsplits every-k {kind} {rows} float32: worst err / bound {worst:.4f}')
    if not ok:                                              # which k classes are wrong: the worst rows, as k, k % N1-candidates are read off k
        want = cell.want(idx)
        want = torch.stack([want.real, want.imag]) if want.is_complex() else want
        err = (got.cpu().double() - want).abs().amax(-1).reshape(-1, rows).amax(0)
        bad = idx[err > 3e-6 * float(want.abs().max())]
        print(f'{bad.numel()} of {rows} k beyond the bound, the first (sorted): {sorted(bad.tolist())[:32]}')
    assert ok, (kind, rows, worst)
    if kind == 'dft':
        at = torch.cat([(idx == 0).nonzero().flatten(), (idx == rows // 2).nonzero().flatten()]).to(DEV)
        assert at.numel() == 2 and bool((got[1, at] == 0).all()), (rows, got[1, at].abs().max())


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_every_dtype_instantiation_is_the_float64_transform(cell):
    """500 random rows with duplicates plus the corners 0, rows / 2, 1, rows - 1; fp32 / fp16 / bf16 input; 'dct': the result in the input's
    dtype; 'dft': planes in fp32 and in the input's dtype.  A fp32 result from 16-bit input has the fp32 bound (the inputs are exact)."""
    kind, rows = cell.kind, cell.rows
    idx = torch.cat([torch.randint(0, rows, (500, ), generator=torch.Generator().manual_seed(rows + 1)), torch.tensor([0, rows // 2, 1, rows - 1])])
    want = cell.want(idx)
    on_device = idx.to(DEV)
    for dtype in DTYPES:
        x = cell.x(dtype)
        for out_dtype in ((dtype, ) if kind == 'dct' or dtype == torch.float32 else (torch.float32, dtype)):
            got = _plain(kind, x, on_device, SCALE, out_dtype)
            assert got.dtype == out_dtype and got.shape == ((2, ) if kind == 'dft' else ()) + (504, cell.features) and got.is_contiguous()
            ok, worst = sampled_rows_check(got, want, ROUNDING[out_dtype])
            print(f'\nsplits dtypes {kind} {rows} {str(dtype)[6:]} -> {str(out_dtype)[6:]}: worst err / bound {worst:.4f}')
            assert ok, (kind, rows, dtype, out_dtype, worst)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_rows_of_a_seed_equal_the_explicit_call_bit_for_bit(cell):
    """sampled_*_seeded(x, p, seed) == sampled_*(x, cabi.sampled_rows(seed, rows, p)) in every dtype; p = 203 (no multiple of 4) and
    p = 5000 (beyond the 4096 rows of one batch); a seed with its top bit set and one without; by value and as an int64 device word"""
    kind, rows = cell.kind, cell.rows
    for dtype in DTYPES:
        x = cell.x(dtype)
        for p in (203, 5000):
            for seed in SEEDS:
                idx = cabi.sampled_rows(seed, rows, p)
                assert idx.shape == (p, ) and 0 <= int(idx.min()) and int(idx.max()) < rows
                want = _plain(kind, x, idx.to(DEV), SCALE)
                assert _same_bits(_seeded(kind, x, p, seed, SCALE), want), (kind, rows, dtype, p, hex(seed), 'by value')
                assert _same_bits(_seeded(kind, x, p, _word(seed), SCALE), want), (kind, rows, dtype, p, hex(seed), 'device word')


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def _valid_counts(rows):
    """prev + 1 (the smallest input the layer routes to `rows`; 1 at 256), rows - 1, the odd rows / 2 - 1, and the even rows / 2 + 2 (the
    first three are all odd: an even one so that Makhoul's map is cut at both parities)"""
    prev = ROWS[ROWS.index(rows) - 1] if rows > ROWS[0] else 0
    return (prev + 1, rows - 1, rows // 2 - 1, rows // 2 + 2)


def test_the_valid_counts_route_to_their_row_count_and_have_both_parities():
    for rows in ROWS:
        low, high, middle, even = _valid_counts(rows)
        assert 1 <= min(low, middle) and max(low, middle, even) < high < rows and len({low, high, middle, even}) == 4, rows
        assert middle % 2 == 1 and high % 2 == 1 and even % 2 == 0, rows
        # the two the layer routes here; the middle one is an input only a direct call hands to this length
        assert cabi_x.sampled_rows_ceil(low) == rows == cabi_x.sampled_rows_ceil(high) and cabi_x.sampled_rows_ceil(low - 1) < rows, rows
    assert _valid_counts(256) == (1, 255, 127, 130) and _valid_counts(768) == (513, 767, 383, 386)


@pytest.mark.parametrize('kind,rows', CELLS, ids=[_cell_id(c) for c in CELLS])
def test_the_zero_extended_pairs_equal_the_plain_ones_on_a_zero_filled_copy_bit_for_bit(kind, rows):
    """x: the first `valid` rows and `features` columns of a rows x ld buffer that is NaN everywhere else (a stray read shows in the
    result: the plain one on the NaN-free copy is finite); every dtype; the four `valid` of _valid_counts (a cut inside every workgroup's
    n1 range for the DFT's order, both parities for Makhoul's map); 64 features behind ld 72 (the buffer-load path of pass A) and 7 behind
    ld 9 (the element path); explicit idx (the corners and 200 random rows) and the rows of a seed"""
    p = 204
    idx = torch.cat([torch.tensor([0, rows - 1, rows // 2, 1]), torch.randint(0, rows, (p - 4, ), generator=torch.Generator().manual_seed(rows))]).to(DEV)
    for features, ld in ((64, 72), (7, 9)):
        data = _integers(rows, features, rows + features).float().to(DEV)
        for dtype in DTYPES:
            for n, valid in enumerate(_valid_counts(rows)):
                buffer = torch.full((rows, ld), float('nan'), dtype=dtype, device=DEV)
                buffer[:valid, :features] = data[:valid]
                x = buffer[:valid, :features]
                padded = torch.zeros(rows, features, dtype=dtype, device=DEV)
                padded[:valid] = x
                seed = SEEDS[n % 2] + rows
                what = (kind, rows, dtype, features, valid)
                assert _same_bits(_zext(kind, x, rows, idx, SCALE), _plain(kind, padded, idx, SCALE)), (*what, 'idx')
                assert _same_bits(_zext_seeded(kind, x, rows, p, seed, SCALE), _seeded(kind, padded, p, seed, SCALE)), (*what, 'seeded')


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
BEYOND = 0xfffffff0                                         # fewbit_fft4.h: kBeyondZext, the bytes a zero-extended pass A addresses
BIG_ROWS, BIG_VALID = 262144, 200000


@pytest.mark.parametrize('dtype,ld', ((torch.bfloat16, 8000), (torch.float32, 4000)), ids=('bfloat16', 'float32'))
@pytest.mark.parametrize('kind', KINDS)
def test_descriptor_offsets_with_the_top_bit_set_and_the_exact_limit_of_the_span(kind, dtype, ld):
    """200000 rows transformed at 262144; x: a 200000 x 64 view of a NaN-filled 200000 x ld buffer of 3.2 GB, so the rows from 134218 on
    lie beyond byte 2^31 of x and their 32-bit buffer offsets have the top bit set.  Every sampled row of the result is a sum over ALL
    source rows, those included: bit-equality with the plain entry point on the compact zero-filled copy (explicit idx and a seed) checks
    them.  Then the largest ld linear._zext_span_ok accepts for 200000 rows (the span ends within a row of 0xfffffff0 bytes): the call runs
    and agrees; with ld + 1 both entry points refuse by name, before any launch.  One allocation of 4.3 GB, viewed three ways, is freed
    at the end."""
    size = torch.empty((), dtype=dtype).element_size()
    limit = BEYOND // (BIG_VALID * size)
    assert linear._zext_span_ok(BIG_VALID, limit, size) and not linear._zext_span_ok(BIG_VALID, limit + 1, size)
    assert 1 << 31 < BIG_VALID * ld * size < BEYOND and ((BIG_VALID - 1) * ld * size) >> 31 == 1
    p, seed = 204, SEEDS[0]
    idx = torch.cat([torch.tensor([0, BIG_ROWS - 1, BIG_ROWS // 2, 1]), torch.randint(0, BIG_ROWS, (p - 4, ), generator=torch.Generator().manual_seed(ld))]).to(DEV)
    data = _integers(BIG_VALID, 64, ld).to(dtype).to(DEV)
    padded = torch.zeros(BIG_ROWS, 64, dtype=dtype, device=DEV)
    padded[:BIG_VALID] = data
    want, want_seeded = _plain(kind, padded, idx, SCALE), _seeded(kind, padded, p, seed, SCALE)
    assert bool(torch.isfinite(want.float()).all())
    flat, x = torch.empty(BIG_VALID * (limit + 1), dtype=dtype, device=DEV), None
    try:
        for stride in (ld, limit):
            flat.fill_(float('nan'))
            x = flat.as_strided((BIG_VALID, 64), (stride, 1))
            x.copy_(data)
            assert x.stride(0) == stride and x.data_ptr() == flat.data_ptr()
            assert _same_bits(_zext(kind, x, BIG_ROWS, idx, SCALE), want), (kind, dtype, stride, 'idx')
            assert _same_bits(_zext_seeded(kind, x, BIG_ROWS, p, seed, SCALE), want_seeded), (kind, dtype, stride, 'seeded')
        x = flat.as_strided((BIG_VALID, 64), (limit + 1, 1))
        assert not linear._zext_span_ok(x.shape[0], x.stride(0), size)
        with pytest.raises(cabi.FewbitHipError, match='4 GiB'):
            _zext(kind, x, BIG_ROWS, idx, SCALE)
        with pytest.raises(cabi.FewbitHipError, match='4 GiB'):
            _zext_seeded(kind, x, BIG_ROWS, p, seed, SCALE)
    finally:
        del flat, x
        torch.cuda.empty_cache()
