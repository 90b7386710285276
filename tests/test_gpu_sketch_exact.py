"""The dense sketch kernels (fewbit_amd/csrc/fewbit_sketch.hip) bit for bit: one-term sums at every tile edge on every kernel variant,
every 16-bit pattern and the fp32 -> bf16 rounding through the operand path, non-finite values confined to their column, the padding
behind `ld`, `out` and the workspace written exactly, results beyond the result dtype's range.

If every column of M holds exactly one nonzero entry, every output is a sum of one product and zeros -- the same bits whatever the stage
order, the slicing or the association of the fp32 sums.  Expected values are float32 arithmetic on the host
(sketch_reference.one_term_expected; tests/test_sketch_exact_host.py ties it to the float64 product, and shows that the schedule and the
settings below leave no row and no kernel variant out).  Rademacher S is the host model's; Gaussian S is fewbit_hip_sketch_matrix's, the
operand as the device rounds it (tests/test_gpu_sketch.py ties that one to the host model)."""
import numpy as np
import pytest
import torch

import sketch_reference as ref
from fewbit_amd import cabi
from helpers import assert_bit_equal, bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
ROWS, ROWS_SLICED = ref.ONE_TERM_ROWS, ref.ONE_TERM_ROWS_SLICED


@pytest.fixture(autouse=True)
def native_sketch_on():
    """these tests are about the gfx950 sketch kernel: select it whatever FEWBIT_SKETCH_NATIVE says in the environment"""
    from fewbit_amd import linear
    prev = linear.use_native_sketch(True)
    yield
    linear.use_native_sketch(prev)


class tuned:
    """the six tune_sketch_* values of a case (a key not named: -1), every one of them back at -1 afterwards"""
    def __init__(self, **tune):
        self.tune = tune

    def __enter__(self):
        for key in ref.TUNE_KEYS:
            getattr(cabi, 'tune_sketch_' + key)(self.tune.get(key, -1))

    def __exit__(self, *exc):
        for key in ref.TUNE_KEYS:
            getattr(cabi, 'tune_sketch_' + key)(-1)
        return False


_MATRICES = {}


def _matrix(dist, dtype, seed, proj, rows):
    """S on the host, float32: the host model (Rademacher, exact), the device's own operand (Gaussian); the largest proj once per key"""
    op = torch.float16 if dtype == torch.float16 else torch.bfloat16
    key = (dist, op if dist == 'gaussian' else None, seed, rows)
    if key not in _MATRICES:
        top = max(ref.ONE_TERM_PROJ)
        _MATRICES[key] = ref.rademacher(seed, top, rows) if dist == 'rademacher' else cabi.sketch_matrix(dist, dtype, seed, top, rows).cpu()
    S = _MATRICES[key]
    assert proj <= S.shape[0]
    return S[:proj]


def _one_term_input(rows, ld, r, values):
    """zeros(rows, ld) on the device with values[f] at (r[f], f); the view of the first len(values) columns"""
    features = values.numel()
    m = torch.zeros(rows, ld, dtype=values.dtype, device=DEV)
    m[torch.as_tensor(r, dtype=torch.int64, device=DEV), torch.arange(features, device=DEV)] = values.to(DEV)
    return m[:, :features]


def _check_one_term(dist, dtype, rows, proj, seed, r, values, scale, ld=None, what=''):
    features = values.numel()
    plan = cabi.describe_sketch(dist, rows, features, proj, dtype)
    got = cabi.sketch(dist, _one_term_input(rows, ld or features, r, values), proj, seed, scale)
    assert got.shape == (proj, features) and got.dtype == dtype
    S = _matrix(dist, dtype, seed, proj, rows)
    want = ref.one_term_expected(S, r, values, scale, bf16_partials=plan['partial_sums'] == 'bf16' and plan['grid'][2] > 1)
    allowance = ref.subnormal_allowance(values, scale) if dist == 'gaussian' else None
    bad = ref.exact_mismatches(got, want, allowance)
    if bool(bad.any()):
        i, f = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f'{what} {dist} {dtype} {rows} x {features} (ld {ld}) proj {proj} scale {scale}: {int(bad.sum())} of {bad.numel()} differ, '
                             f'{int(bad.any(0).sum())} columns, first out[{i}, {f}] = {float(got[i, f])!r}, expected {float(want[i, f])!r} = '
                             f'S[{i}, {int(r[f])}] ({float(S[i, int(r[f])])!r}) x {float(values[f])!r}; plan {plan}')
    return got, want


# ---- 1. one-term sums at every tile edge, on every kernel variant ---------------------------------------------------------------------
@pytest.mark.parametrize('dist,dtype,tune', ref.exact_cases(), ids=lambda v: str(v).replace('torch.', '').replace("'", '').replace(' ', ''))
def test_one_term_sums_are_exact_at_every_tile_edge(dist, dtype, tune):
    """645 rows (3717 too when the setting slices the rows) x 264 / 261 / 520 features, proj 130 / 257, ld = features / features + 3,
    scales 1, -0.5 and 1 / proj: column f holds one randn x 2^e at row 277 (f + features x phase) mod rows, and over the phases every row
    of M is that row for some column.  Each case first asserts that it runs the kernel variant it is named after."""
    with tuned(**tune):
        for rows in ((ROWS, ROWS_SLICED) if tune.get('slices', -1) == 3 else (ROWS, )):
            want = ref.expected_plan(dist, dtype, tune, rows)
            for features in ref.ONE_TERM_FEATURES:
                for proj in ref.ONE_TERM_PROJ:
                    plan = cabi.describe_sketch(dist, rows, features, proj, dtype)
                    assert ('128x512' in plan['kernel']) == want['wide'] and (want['tile'] + ' tile') in plan['kernel'], (plan, tune)
                    assert ('from memory' in plan['kernel']) == want['from_memory'], (plan, tune)
                    assert plan['converted_to_bf16_first'] is want['converted'], (plan, tune)
                    assert plan['grid'][2] == want['gz'] and plan['partial_sums'] == want['partial_sums'], (plan, tune)
                    for phase in range(ref.one_term_phases(rows, features)):
                        ld = features + 3 * ((phase + proj) % 2)
                        scale = ref.ONE_TERM_SCALES[(phase + features) % 3] or 1.0 / proj
                        r = ref.one_term_rows(rows, features, phase)
                        values = ref.one_term_values(features, dtype, 1000 * features + phase)
                        _check_one_term(dist, dtype, rows, proj, 0xfeed + rows, r, values, scale, ld, what=f'phase {phase} {tune}')


# ---- 2. every 16-bit pattern through the operand path ---------------------------------------------------------------------------------
def _subnormal(t):
    return (t != 0) & (t.abs() < torch.finfo(t.dtype).smallest_normal)


@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float16))
def test_every_16_bit_pattern_goes_through_the_operand_path_unchanged(dtype):
    """M = zeros(136, 65536) with all 65536 patterns in one row -- once in the full first stage, once in the partial last stage (rows
    128 ... 135) -- Rademacher, proj 33, scale 1, both tile heights: out[i, f] = S[i, r] x pattern exactly.  Subnormals come out as
    subnormals, +-Inf as +-Inf with the sign of S, every NaN pattern as a NaN."""
    rows, features, proj, seed = 136, 65536, 33, 20260701
    patterns = torch.arange(features, dtype=torch.int32).to(torch.int16).view(dtype)
    S = ref.rademacher(seed, proj, rows)
    for waves in (4, 8):
        with tuned(waves=waves, halves=1):
            assert cabi.describe_sketch('rademacher', rows, features, proj, dtype)['threads'] == 64 * waves
            for row in (5, 133):
                r = np.full(features, row)
                got, want = _check_one_term('rademacher', dtype, rows, proj, seed, r, patterns, 1.0, what=f'waves {waves} row {row}')
                # (what the expected value amounts to, spelled out)
                sub, nan, inf = _subnormal(patterns), torch.isnan(patterns), torch.isinf(patterns)
                assert int(sub.sum()) == 2 * (2**(7 if dtype == torch.bfloat16 else 10) - 1) and int(nan.sum()) == int(sub.sum()) and int(inf.sum()) == 2
                g = got.cpu()
                assert bool((g[:, sub].float() == S[:, row:row + 1] * patterns[sub].float()[None, :]).all()) and bool((g[:, sub] != 0).all())
                assert bool(torch.isnan(g[:, nan]).all())
                assert bool((g[:, inf].float() == S[:, row:row + 1] * patterns[inf].float()[None, :]).all())


# ---- 3. fp32 -> bf16 rounding ----------------------------------------------------------------------------------------------------------
LOW_HALVES = (0, 1, 0x7fff, 0x8000, 0x8001, 0xffff)


def _f32_patterns(upper, lower):
    """upper halves (an int64 tensor) x 2^16 + lower halves (an int, or a tensor of the same length), as float32"""
    return ((upper << 16) | lower).to(torch.int32).view(torch.float32)


@pytest.mark.parametrize('convert', (0, 1))
def test_fp32_is_rounded_to_bf16_to_nearest_even_wherever_it_is_converted(convert):
    """every upper half b with the lower halves 0, 1, 0x7fff, 0x8000, 0x8001, 0xffff, laid out as the 16-bit patterns above; Rademacher,
    scale 1, fp32 result = S[i, r] x float32(bf16(x)): ties to even, rounding up across a binade, 0x7f7f8000 and above -> Inf, subnormals,
    every NaN (0x7f800001 too) a NaN.  convert = 0: the staging of the product kernel, convert = 1: to_bf16_kernel; 65533 features: the
    element-wise guarded path of each."""
    rows, proj, seed = 136, 33, 20260702
    upper = torch.arange(65536, dtype=torch.int64)
    with tuned(convert=convert):
        for features, lowers in ((65536, LOW_HALVES), (65533, (None, ))):
            assert cabi.describe_sketch('rademacher', rows, features, proj, torch.float32)['converted_to_bf16_first'] is bool(convert)
            for k, low in enumerate(lowers):
                if low is None:                            # every lower half in one call, upper halves 0 ... 65532
                    low = torch.tensor(LOW_HALVES, dtype=torch.int64)[upper[:features] % len(LOW_HALVES)]
                x = _f32_patterns(upper[:features], low)
                for row in (5, 133):
                    _check_one_term('rademacher', torch.float32, rows, proj, seed, np.full(features, row), x, 1.0, what=f'convert {convert} low {k} row {row}')
    # the reference conversion itself, on the cases named above
    x = torch.tensor([0x3f808000, 0x3f818000, 0x3f7fffff, 0x7f7f8000, 0x7f7f7fff, 0x7f800001, 0x00008000, 0x00018000], dtype=torch.int32).view(torch.float32)
    assert (x.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xffff).tolist()[:5] == [0x3f80, 0x3f82, 0x3f80, 0x7f80, 0x7f7f]
    assert bool(torch.isnan(x.to(torch.bfloat16)[5])) and (x.to(torch.bfloat16).view(torch.int16)[6:]).tolist() == [0, 2]


# ---- 4. a non-finite value stays in its column ------------------------------------------------------------------------------------------
def _pattern(t):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf"""
    t = t.double()
    return torch.isnan(t) * 1 + (t == float('inf')) * 2 + (t == -float('inf')) * 3


@pytest.mark.parametrize('dist', cabi.SKETCH_DISTS)
@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_a_non_finite_value_stays_in_its_column(dist, dtype):
    """NaN, +Inf or -Inf at one entry of a randn M (and +Inf at two rows of one column): every other output column is bit-identical to the call
    on the clean input, the column itself has exactly the NaN / +Inf / -Inf pattern of the float64 product S @ op(M).  Column 0 is what
    tile columns beyond the matrix are read from, the last row what rows beyond the last stage are clamped to.  The policy at 645 rows and
    three slices at 3717 rows (645 rows are never sliced), 261 and 520 features, proj 130."""
    proj, seed = 130, 77
    for rows, tune in ((ROWS, {}), (ROWS_SLICED, dict(slices=3))):
        S = _matrix(dist, dtype, seed, proj, rows).double()
        for features in (261, 520):
            with tuned(**tune):
                assert cabi.describe_sketch(dist, rows, features, proj, dtype)['grid'][2] == (3 if tune else 1)
                clean = torch.randn(rows, features, generator=torch.Generator().manual_seed(rows + features)).to(dtype)
                base = cabi.sketch(dist, clean.to(DEV), proj, seed, 0.5)
                assert bool(torch.isfinite(base).all())
                spots = [((0, 0), ), ((rows - 1, 0), ), ((rows - 1, features - 1), ), ((300, 255), ), ((300, 256), ), ((rows - 5, features - 3), )]
                cases = [(spot, value) for spot in spots for value in (float('nan'), float('inf'), -float('inf'))]
                cases.append((((3, 17), (rows - 2, 17)), float('inf')))
                cases.append((((0, 0), (rows - 300, 0)), float('inf')))
                for spot, value in cases:
                    m = clean.clone()
                    for (row, col) in spot:
                        m[row, col] = value
                    col = spot[0][1]
                    got = cabi.sketch(dist, m.to(DEV), proj, seed, 0.5)
                    others = [c for c in range(features) if c != col]
                    assert_bit_equal(got[:, others], base[:, others], f'{dist} {dtype} {rows} x {features} {spot} = {value}', nan_equal=False)
                    want = 0.5 * (S @ ref.operand(m[:, col:col + 1]).double())[:, 0]
                    assert int((_pattern(want) != 0).sum()) > 0
                    assert torch.equal(_pattern(got[:, col].cpu()), _pattern(want)), (dist, dtype, rows, features, spot, value)


# ---- 5. the padding behind ld is never used ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dist', cabi.SKETCH_DISTS)
@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_the_padding_behind_ld_is_never_used(dist, dtype):
    """NaN, Inf and 1e30 in the columns features ... ld - 1, ld - features = 1, 3, 8: bit-identical to the call on a contiguous copy"""
    rows, proj, seed = ROWS, 130, 78
    for convert in ((0, 1) if dtype == torch.float32 else (-1, )):
        with tuned(convert=convert):
            for features in (261, 264):
                plain = torch.randn(rows, features, generator=torch.Generator().manual_seed(features)).to(dtype).to(DEV)
                want = cabi.sketch(dist, plain, proj, seed, -0.5)
                assert bool(torch.isfinite(want).all())
                for pad in (1, 3, 8):
                    for fill in (float('nan'), float('inf'), 1e30):
                        wide = torch.full((rows, features + pad), fill).to(dtype).to(DEV)
                        wide[:, :features] = plain
                        view = wide[:, :features]
                        assert view.stride(0) == features + pad
                        assert_bit_equal(cabi.sketch(dist, view, proj, seed, -0.5), want, f'{dist} {dtype} {features} + {pad}, {fill}, convert {convert}',
                                         nan_equal=False)


# ---- 6. out and the workspace are written exactly -----------------------------------------------------------------------------------------
WRITTEN_EXACTLY = (                                       # (what, distribution, dtype, features, tune)
    ('three slices, fp32 partial sums', 'rademacher', torch.bfloat16, 264, dict(slices=3, partials=0)),
    ('three slices, fp32 partial sums (fp16)', 'gaussian', torch.float16, 264, dict(slices=3, materialise=0)),
    ('three slices, bf16 partial sums', 'rademacher', torch.bfloat16, 264, dict(slices=3, partials=1)),
    ('three slices, bf16 partial sums, ragged', 'gaussian', torch.bfloat16, 261, dict(slices=3, partials=1, materialise=0)),
    ('Gaussian from memory', 'gaussian', torch.bfloat16, 264, dict(slices=1, materialise=1)),
    ('Gaussian from memory, three slices, ragged', 'gaussian', torch.float16, 261, dict(slices=3, materialise=1)),
    ('fp32 converted first', 'rademacher', torch.float32, 264, dict(slices=1, convert=1)),
    ('fp32 converted first, from memory, bf16 partial sums, ragged', 'gaussian', torch.float32, 261, dict(slices=3, convert=1, partials=1, materialise=1)),
    ('no workspace, ragged', 'rademacher', torch.float16, 261, dict(slices=1)),
    ('fp32 staged in the kernel, ragged', 'gaussian', torch.float32, 261, dict(slices=1, convert=0)),
)


@pytest.mark.parametrize('what,dist,dtype,features,tune', WRITTEN_EXACTLY, ids=[c[0].replace(' ', '_') for c in WRITTEN_EXACTLY])
def test_out_and_the_workspace_are_written_exactly(what, dist, dtype, features, tune):
    """`out` a view in the middle of a buffer of 0xa5 bytes, an odd number of elements in (a 16-bit `out` is 2-byte aligned only), prefilled
    with NaN: the bytes around it unchanged, no NaN left, the bits of the call that allocates its own.  The workspace of exactly
    sketch_workspace_bytes(...) bytes, 256-byte aligned, inside a buffer of sentinel bytes, once prefilled with 0xff bytes (NaN as a partial
    sum, as a bf16 copy, as a fragment) and once with zeros: the same bits both times -- nothing is read before it is written -- and the
    sentinels intact."""
    rows, proj, seed = ROWS_SLICED, 130, 79
    m = torch.randn(rows, features, generator=torch.Generator().manual_seed(features)).to(dtype).to(DEV)
    with tuned(**tune):
        plan = cabi.describe_sketch(dist, rows, features, proj, dtype)
        need = cabi.sketch_workspace_bytes(dist, rows, features, proj, dtype)
        assert plan['grid'][2] == tune['slices'] and need == plan['workspace_bytes']
        assert ('from memory' in plan['kernel']) == (tune.get('materialise') == 1) and plan['converted_to_bf16_first'] is (tune.get('convert') == 1)
        if 'partial sums' in what:
            assert plan['partial_sums'] == ('bf16' if 'bf16 partial' in what else 'fp32')
        assert (need == 0) == ('no workspace' in what or 'staged' in what)
        want = cabi.sketch(dist, m, proj, seed, 0.25)
        assert bool(torch.isfinite(want).all())
        size = want.element_size()
        lead, tail, nbytes = 3 * size, 1031 * size, proj * features * size
        results = []
        for fill in (0xff, 0x00):
            buf = torch.full((lead + nbytes + tail, ), 0xa5, dtype=torch.uint8, device=DEV)
            out = buf[lead:lead + nbytes].view(dtype).view(proj, features)
            out.fill_(float('nan'))
            wbuf = torch.full((512 + need + 256, ), 0x5a, dtype=torch.uint8, device=DEV)
            fence = 256 + (-wbuf.data_ptr()) % 256
            workspace = wbuf[fence:fence + need]
            workspace.fill_(fill)
            assert (need == 0 or workspace.data_ptr() % 256 == 0) and out.data_ptr() % (2 * size) == size
            y = cabi.sketch(dist, m, proj, seed, 0.25, out=out, workspace=workspace if need else None)
            assert y.data_ptr() == out.data_ptr()
            assert bool((buf[:lead] == 0xa5).all()) and bool((buf[lead + nbytes:] == 0xa5).all()), (what, fill)
            assert bool((wbuf[:fence] == 0x5a).all()) and bool((wbuf[fence + need:] == 0x5a).all()), (what, fill)
            assert not bool(torch.isnan(out).any()), (what, fill)
            results.append(out.clone())
        assert torch.equal(bits(results[0]), bits(results[1])), what
        assert torch.equal(bits(results[0]), bits(want)), what


# ---- 7. results beyond the result dtype's range ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dist', cabi.SKETCH_DISTS)
@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_results_beyond_the_range_of_the_result_dtype_are_the_right_infinity(dist, dtype):
    """one-term inputs around the top of the range -- the scaled product beyond 65504 (fp16), beyond 2^128 (bf16 and fp32: the fp32 product
    with the scale overflows; bf16 partial sums and the fp32 -> bf16 rounding of M may overflow before it): the Inf of the right sign where
    the float32 formula gives one, the exact finite value next to it"""
    features, proj, seed = 264, 130, 80
    g = torch.Generator().manual_seed(7)
    top = 2.0**14 if dtype == torch.float16 else 2.0**126
    sign = torch.where(torch.rand(features, generator=g) < 0.5, -1.0, 1.0)
    values = (sign * top * (1.0 + 2.9 * torch.rand(features, generator=g))).to(dtype)              # [1, 3.9) x top
    values[:4] = torch.tensor([top * 2 * (2 - 2.0**-7), -top * 2 * (2 - 2.0**-7), top, -top]).to(dtype)
    assert bool(torch.isfinite(values).all())
    settings = [(ROWS, {}, 2.0)]
    if dtype != torch.float16:
        settings.append((ROWS_SLICED, dict(slices=3, partials=1, convert=1), 1.5))
    if dtype == torch.float32:
        values[4:8] = torch.tensor([0x7f7f8000, 0x7f7f7fff, 0xff7f8000 - 2**32, 0xff7fffff - 2**32], dtype=torch.int32).view(torch.float32)
        settings.append((ROWS, dict(convert=0), 2.0))
    for rows, tune, scale in settings:
        with tuned(**tune):
            for phase in range(3):
                r = ref.one_term_rows(rows, features, phase)
                got, want = _check_one_term(dist, dtype, rows, proj, seed, r, values, scale, what=f'{tune}')
                inf = torch.isinf(want)
                assert float(inf.float().mean()) > 0.2 and bool((want[inf] > 0).any()) and bool((want[inf] < 0).any())
                assert bool(torch.isfinite(want).any()) and not bool(torch.isnan(want).any())
