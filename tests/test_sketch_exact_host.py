"""What tests/test_gpu_sketch_exact.py relies on, checked without a GPU: the one-nonzero-per-column schedule reaches every row of M and both
sides of every tile boundary, the list of tuning settings reaches every kernel variant of every distribution and dtype (through
fewbit_hip_sketch_describe, which answers without a device: 256 CUs assumed), and the expected value of a one-term output is the float64
product rounded once."""
import ctypes
import json

import numpy as np
import pytest
import torch

import sketch_reference as ref
from fewbit_amd import cabi

ROW_COUNTS = (ref.ONE_TERM_ROWS, ref.ONE_TERM_ROWS_SLICED)


def _tune(L, tune):
    for key in ref.TUNE_KEYS:
        assert L.fewbit_hip_tune(('sketch_' + key).encode(), int(tune.get(key, -1))) == 0, L.fewbit_hip_last_error()


def _describe(L, dist, dtype, rows, features, proj):
    buf = ctypes.create_string_buffer(512)
    assert L.fewbit_hip_sketch_describe(cabi.SKETCH_DISTS.index(dist), cabi.DTYPES[dtype], rows, features, proj, buf, len(buf)) == 0
    return json.loads(buf.value.decode())


@pytest.fixture()
def L():
    lib = cabi.lib()
    try:
        yield lib
    finally:
        _tune(lib, {})


@pytest.mark.parametrize('rows', ROW_COUNTS)
@pytest.mark.parametrize('features', ref.ONE_TERM_FEATURES)
def test_the_schedule_makes_every_row_the_nonzero_row_of_some_column(rows, features):
    """(a) 277 is coprime to the row count, so column f + features * phase -> 277 (f + features * phase) mod rows is one-to-one on
    [0, rows): ceil(rows / features) calls cover every row -- and so the row on each side of every boundary of a 64- or 128-row stage, a
    256-row Rademacher block, a 1280-row slice and the end of the matrix"""
    assert np.gcd(ref.ONE_TERM_STEP, rows) == 1
    phases = ref.one_term_phases(rows, features)
    assert phases >= -(-rows // features) and phases >= len(ref.ONE_TERM_SCALES)
    hit = np.zeros(rows, dtype=np.int64)
    for phase in range(phases):
        r = ref.one_term_rows(rows, features, phase)
        assert r.shape == (features, ) and r.min() >= 0 and r.max() < rows
        hit[r] += 1
    assert bool((hit > 0).all())
    for tile in (64, 128, 256, 1280):
        for edge in range(tile, rows, tile):
            assert hit[edge - 1] > 0 and hit[edge] > 0, (tile, edge)
    assert hit[0] > 0 and hit[rows - 1] > 0
    assert rows % 256 == 128 + 5                   # the last 64-row stage holds 5 valid rows, the last 128-row stage 128 + 5 ...
    last = rows - rows % 64
    assert all(hit[last:rows] > 0) and rows - last == 5


def test_the_sliced_row_count_is_three_slices_of_whole_blocks(L):
    _tune(L, dict(slices=3))
    for dist, dtype, _ in ref.exact_cases():
        plan = _describe(L, dist, dtype, ref.ONE_TERM_ROWS_SLICED, 264, 130)
        assert plan['grid'][2] == 3 and plan['k_slice'] == 1280, plan
        assert _describe(L, dist, dtype, ref.ONE_TERM_ROWS, 264, 130)['grid'][2] == 1        # (fewer than 1024 rows: never sliced)


def test_the_settings_reach_every_kernel_variant_of_every_distribution_and_dtype(L):
    """(b) the union of the plans over EXACT_SETTINGS x shapes, per distribution and dtype; every plan is also what expected_plan says,
    the fields the GPU sweep asserts case by case"""
    seen = {}
    for dist, dtype, tune in ref.exact_cases():
        _tune(L, tune)
        rows_of = ROW_COUNTS if tune.get('slices', -1) == 3 else (ref.ONE_TERM_ROWS, )
        for rows in rows_of:
            want = ref.expected_plan(dist, dtype, tune, rows)
            for features in ref.ONE_TERM_FEATURES:
                for proj in ref.ONE_TERM_PROJ:
                    plan = _describe(L, dist, dtype, rows, features, proj)
                    assert (want['tile'] + ' tile') in plan['kernel'] and ('from memory' in plan['kernel']) == want['from_memory'], (plan, tune)
                    assert plan['converted_to_bf16_first'] is want['converted'] and plan['grid'][2] == want['gz'], (plan, tune)
                    assert plan['partial_sums'] == want['partial_sums'], (plan, tune, dist, dtype)
                    tags = seen.setdefault((dist, dtype), set())
                    tags.add(want['tile'])
                    if want['from_memory']:
                        tags.add('from memory')
                    if want['converted']:
                        tags.add('converted')
                    if features % 8:
                        tags.add('ragged')
                        tags.add('ragged ' + want['tile'])
                    if plan['grid'][2] > 1:
                        tags.add('sliced ' + plan['partial_sums'])
    for dist in cabi.SKETCH_DISTS:
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            need = {'128x256', '256x256', '128x512', 'ragged', 'ragged 128x256', 'ragged 256x256', 'ragged 128x512', 'sliced fp32'}
            if dist == 'gaussian':
                need.add('from memory')
            if dtype == torch.float32:
                need.add('converted')
            if dtype != torch.float16:                     # (fp16 keeps fp32 partial sums: range)
                need.add('sliced bf16')
            assert need <= seen[(dist, dtype)], (dist, dtype, need - seen[(dist, dtype)])


@pytest.mark.parametrize('dist', cabi.SKETCH_DISTS)
@pytest.mark.parametrize('dtype', (torch.float32, torch.float16, torch.bfloat16))
def test_the_expected_value_is_the_float64_product_rounded_once(dist, dtype):
    """(c) on the host model's S: wherever S[i, r] * op(m) * float32(scale) is a float32 number, the helper's float32 arithmetic equals
    the float64 product rounded once to the dtype of M (and that is nearly everywhere for the scales 1 and -0.5)"""
    rows, features, proj = ref.ONE_TERM_ROWS, 261, 130
    S = ref.matrix(dist, 12345, proj, rows, dtype)
    for phase, scale in enumerate((1.0, -0.5, 1.0 / proj)):
        r = ref.one_term_rows(rows, features, phase)
        values = ref.one_term_values(features, dtype, phase)
        values[7] = 0.0
        values[8] = -0.0
        got = ref.one_term_expected(S, r, values, scale)
        assert got.dtype == dtype and got.shape == (proj, features)
        m = torch.zeros(rows, features, dtype=torch.float64)
        m[torch.from_numpy(r), torch.arange(features)] = ref.operand(values).double()
        product = (S.double() @ m) * float(torch.tensor(scale, dtype=torch.float32))
        exact = product.float().double() == product
        assert float(exact.double().mean()) > (0.99 if scale != 1.0 / proj else 0.001)
        once = product.float().to(dtype)                   # (exact in float32 where it counts: one rounding, to `dtype`)
        bad = ref.exact_mismatches(got, once) & exact
        assert not bool(bad.any()), (dist, dtype, scale, int(bad.sum()))
        assert bool((got[:, 7:9] == 0).all())


def test_the_comparison_is_bit_for_bit_but_for_nan_payloads_and_the_sign_of_zero():
    a = torch.tensor([1.0, float('nan'), 0.0, -0.0, float('inf'), 1.0, 2.0**-140])
    b = torch.tensor([1.0, float('nan'), -0.0, 0.0, float('inf'), 1.0 + 2.0**-23, 2.0**-140 + 2.0**-149])
    b.view(torch.int32)[1] = 0x7f800001                   # another NaN
    assert ref.exact_mismatches(a, b).tolist() == [False, False, False, False, False, True, True]
    allow = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0**-149], dtype=torch.float64)
    assert ref.exact_mismatches(a, b, allow).tolist() == [False, False, False, False, False, True, False]
    assert ref.exact_mismatches(torch.tensor([float('inf')]), torch.tensor([-float('inf')])).tolist() == [True]
    assert ref.exact_mismatches(torch.tensor([float('nan')]), torch.tensor([float('inf')])).tolist() == [True]
    tiny = ref.subnormal_allowance(torch.tensor([1.0, 2.0**-101, -2.0**-120]), -0.5)
    assert tiny.tolist() == [[0.0, 2.0**-150, 2.0**-150]]
