"""The plan of a dense sketch call (fewbit_amd/csrc/fewbit_sketch.hip: tile, grid, row slices, partial sums, workspace parts) without a GPU:
what fewbit_hip_sketch_describe writes and fewbit_hip_sketch_workspace returns, against tests/golden/sketch_plans.json -- the answers of the
library built from the commit that file names, recorded by tests/golden/gen_sketch_plans.py.  The host side may be rearranged; the plan of a
call may not move: the strings are compared as written (not parsed), under the built-in policy and under every tuning setting of the table.

Both entry points answer without a device (256 CUs assumed, what an MI355X reports), so the C entry points are called through cabi.lib()
directly: cabi.describe_sketch wants a current CUDA device."""
import ctypes
import hashlib
import itertools
import json

import pytest
import torch

from fewbit_amd import cabi
from helpers import GOLDEN

TABLE = GOLDEN / 'sketch_plans.json'
KEYS = ('sketch_slices', 'sketch_waves', 'sketch_halves', 'sketch_convert', 'sketch_partials', 'sketch_materialise')
DISTS = cabi.SKETCH_DISTS                                  # enum fewbit_sketch_dist
DTYPES = ('f32', 'f16', 'bf16')                            # enum fewbit_dtype: 0, 1, 2


def tune(L, setting):
    """all six keys, every time: the ones a setting does not name are back at the built-in policy"""
    for key in KEYS:
        assert L.fewbit_hip_tune(key.encode(), int(setting.get(key, -1))) == 0, L.fewbit_hip_last_error()


def answers(L, dist, dtype, shape):
    """-> (the describe string as written, the workspace size) of one call.  rows == 0: the workspace size alone (string None) -- the
    library the table was recorded from divided by zero when asked to describe a call without rows, so there is no string to hold on to;
    test_an_empty_call_is_described_too says what is expected there."""
    workspace = int(L.fewbit_hip_sketch_workspace(dist, dtype, *shape))
    if shape[0] == 0:
        return None, workspace
    buf = ctypes.create_string_buffer(512)
    assert L.fewbit_hip_sketch_describe(dist, dtype, *shape, buf, len(buf)) == 0, L.fewbit_hip_last_error()
    return buf.value.decode(), workspace


def digest(L, dist, dtype, shapes):
    h = hashlib.sha256()
    for shape in shapes:
        text, workspace = answers(L, dist, dtype, shape)
        h.update(('%d %d %d %d %s\n' % (*shape, workspace, text)).encode())
    return h.hexdigest()


def all_shapes(table):
    """the shapes behind a digest: the listed ones, then the two cross products (thresholds of the policy; the edges of the GPU fuzz test)"""
    return ([tuple(s) for s in table['shapes']] + list(itertools.product(*table['threshold_cross']))
            + list(itertools.product(*table['fuzz_cross'])))


@pytest.fixture(scope='module')
def table():
    return json.loads(TABLE.read_text())


@pytest.fixture()
def L(table):
    if torch.cuda.is_available():
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        if cus != table['cus']:
            pytest.skip(f"this GPU reports {cus} CUs; the table was recorded for {table['cus']}")
    lib = cabi.lib()
    try:
        yield lib
    finally:
        tune(lib, {})


def test_the_table_covers_what_it_must(table):
    """the grid itself: both distributions x three dtypes in every group, every key at non-default values alone, the combinations of the GPU
    tests, the shapes of tests/test_gpu_sketch.py and both sides of the policy's thresholds"""
    groups = {f'{d}/{t}' for d in DISTS for t in DTYPES}
    assert set(table['default']) == groups and all(set(s['digests']) == groups for s in table['settings'])
    assert all(len(v) == len(table['shapes']) for v in table['default'].values())
    alone = {key: {s['tune'][key] for s in table['settings'] if list(s['tune']) == [key]} for key in KEYS}
    assert alone['sketch_waves'] == {4, 8} and alone['sketch_halves'] == {1, 2} and alone['sketch_convert'] == {0, 1}
    assert alone['sketch_partials'] == {0, 1, 2} and alone['sketch_materialise'] == {0, 1}
    assert {1, 2, 3, 4, 7, 8, 16, 17} <= alone['sketch_slices']                 # (any count > 0 is legal: the ones the tests use, the cap of 16, one past it)
    tunes = [s['tune'] for s in table['settings']]
    assert any(t.get('sketch_waves') == 8 and t.get('sketch_halves') == 1 and t.get('sketch_slices', -1) > 1 for t in tunes)
    assert {'sketch_halves': 2, 'sketch_materialise': 0} in tunes and {} in tunes
    shapes = set(all_shapes(table))
    for shape in ((16384, 3072, 1638), (16384, 768, 3276), (2**21, 768, 2**10), (2**20 + 3, 264, 200), (70000, 40, 1290), (8192, 392, 1400), (2049, 520, 257)):
        assert list(shape) in table['shapes']
    for rows, features, proj in itertools.product((1023, 1024), (256, 257, 1023, 1024, 2047, 2048, 1536, 2304), (1280, 1281)):
        assert (rows, features, proj) in shapes
    assert any(r >= 16 * 1024 and f <= 256 and p <= 128 for r, f, p in shapes)                       # 16 slices
    assert {(0, 16, 4), (16, 0, 4), (16, 8, 0)} <= shapes


def test_the_default_policy_string_for_string(L, table):
    tune(L, {})
    shapes = [tuple(s) for s in table['shapes']]
    for d, dist in enumerate(DISTS):
        for t, dtype in enumerate(DTYPES):
            want = table['default'][f'{dist}/{dtype}']
            for shape, (text, workspace) in zip(shapes, want):
                assert answers(L, d, t, shape) == (text, workspace), (dist, dtype, shape)
    # the figures quoted where the table was asked for: rademacher, fp32, 16384 x 3072, p = 1638
    text, workspace = answers(L, 0, 0, (16384, 3072, 1638))
    assert '"grid": [12, 7, 3]' in text and '"k_slice": 5632' in text and workspace == 130854912


def test_an_empty_call_is_described_too(L):
    """rows == 0 (the entry point writes zeros and launches no product): one slice, no workspace, no conversion, no fragments"""
    tune(L, {})
    for d, t, features, proj in itertools.product(range(2), range(3), (16, 3072), (4, 3276)):
        buf = ctypes.create_string_buffer(512)
        assert L.fewbit_hip_sketch_describe(d, t, 0, features, proj, buf, len(buf)) == 0
        plan = json.loads(buf.value.decode())
        assert plan['grid'][2] == 1 and plan['workspace_bytes'] == 0 == L.fewbit_hip_sketch_workspace(d, t, 0, features, proj)
        assert plan['converted_to_bf16_first'] is False and plan['partial_sums'] is None and plan['s_fragment_bytes'] == 0


def test_every_tuning_setting_by_digest(L, table):
    shapes = all_shapes(table)
    wrong = []
    for setting in table['settings']:
        tune(L, setting['tune'])
        for d, dist in enumerate(DISTS):
            for t, dtype in enumerate(DTYPES):
                if digest(L, d, t, shapes) != setting['digests'][f'{dist}/{dtype}']:
                    wrong.append((setting['tune'], dist, dtype))
    assert not wrong, wrong


def test_the_fuzz_cases_of_the_gpu_suite(L, table):
    """the 60 (shape, dtype, six tuning values) draws of tests/test_gpu_sketch.py::test_seeded_fuzz_of_shapes_dtypes_strides_and_tiles"""
    assert len(table['fuzz_cases']) == 60
    for case in table['fuzz_cases']:
        tune(L, case['tune'])
        assert answers(L, case['dist'], case['dtype'], tuple(case['shape'])) == (case['describe'], case['workspace']), case
