"""The companion library libfewbit_hipx.so (include/fewbit_hipx.h) without a GPU: it loads, exports exactly what its header declares,
reports version 1, and its workspace is a host-side formula (the sampled DCT's); libfewbit_hip.so still exports the frozen ABI-5 list."""
import ctypes
import re
import subprocess
import sys

import pytest
import torch

from fewbit_amd import cabi, cabi_x
from helpers import ROOT

# the frozen C-ABI of libfewbit_hip.so (FEWBIT_HIP_ABI_VERSION 5; also pinned by tests/test_api.py): the new entry points must not land there
FROZEN_ABI = '''
fewbit_hip_abi_version fewbit_hip_last_error fewbit_hip_bitwidth fewbit_hip_state_nbytes
fewbit_hip_quantize_forward fewbit_hip_quantize_backward fewbit_hip_stepwise1_forward fewbit_hip_stepwise1_backward
fewbit_hip_pack_codes fewbit_hip_unpack_codes
fewbit_hip_describe_quantize_forward fewbit_hip_describe_quantize_backward fewbit_hip_describe_stepwise1_forward
fewbit_hip_describe_stepwise1_backward fewbit_hip_tune
fewbit_hip_sketch_workspace fewbit_hip_sketch fewbit_hip_sketch_device_seed fewbit_hip_sketch_next_seed fewbit_hip_sketch_mix_seed
fewbit_hip_sketch_matrix fewbit_hip_sketch_describe fewbit_hip_philox4x32 fewbit_hip_xoshiro128pp
fewbit_hip_sampled_dct_workspace fewbit_hip_sampled_dct fewbit_hip_sampled_dct_seeded fewbit_hip_sampled_rows
'''.split()


def _exported(path):
    out = subprocess.run(['nm', '-D', '--defined-only', str(path)], check=True, capture_output=True, text=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_the_companion_library_loads_and_reports_version_1():
    assert cabi_x.LIB_PATH.name == 'libfewbit_hipx.so' and cabi_x.LIB_PATH.parent == cabi.LIB_PATH.parent
    ctypes.CDLL(str(cabi_x.LIB_PATH))
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    version = int(re.search(r'#define FEWBIT_HIPX_ABI_VERSION (\d+)', header).group(1))
    assert cabi_x.lib().fewbit_hipx_abi_version() == version == cabi_x.ABI_VERSION == 1


def test_the_companion_library_exports_exactly_what_its_header_declares():
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    declared = sorted(set(re.findall(r'\b(fewbit_hipx_\w+)\s*\(', header)))
    assert declared == sorted(cabi_x.SYMBOLS)
    assert _exported(cabi_x.LIB_PATH) == declared


def test_the_frozen_library_still_exports_the_abi_5_list():
    assert _exported(cabi.LIB_PATH) == sorted(FROZEN_ABI) == sorted(cabi.SYMBOLS)
    assert cabi.lib().fewbit_hip_abi_version() == 5


SUPPORTED = [1 << k for k in range(8, 19)] + [3 << k for k in range(8, 15)] + [5 << k for k in range(8, 14)]


@pytest.mark.parametrize('dtype', (torch.float32, torch.float16, torch.bfloat16))
def test_the_workspace_is_the_dct_formula_for_every_supported_shape(dtype):
    for rows in SUPPORTED:
        for features, proj in ((1, 1), (64, 10), (770, 3276), (3072, rows // 5)):
            want = cabi.sampled_dct_workspace_bytes(rows, features, proj, dtype)
            assert want == -(-features // 64) * rows * 256 + 2048 + -(-8 * proj // 16) * 16
            assert cabi_x.sampled_dft_workspace_bytes(rows, features, proj, dtype) == want, (rows, features, proj)


def test_shapes_without_a_kernel_have_no_workspace():
    for rows in (0, 48, 128, 255, 3000, 1792, 81920, 98304, 524288):
        assert cabi_x.sampled_dft_workspace_bytes(rows, 64, 10) == 0, rows
    assert cabi_x.sampled_dft_workspace_bytes(1024, 64, 10, torch.float64) == 0
    assert cabi_x.sampled_dft_workspace_bytes(1024, 0, 10) == 0 == cabi_x.sampled_dft_workspace_bytes(1024, 64, 0)
    assert cabi_x.lib().fewbit_hipx_sampled_dft_workspace(7, 1024, 64, 10) == 0          # (an unknown dtype, at the C level)


def test_calls_are_refused_by_name_before_anything_is_launched():
    L = cabi_x.lib()
    # an unknown dtype, an out_dtype that is neither F32 nor the input's, unsupported rows, a misaligned seed word: refused on the host
    assert L.fewbit_hipx_sampled_dft(9, None, 1024, 8, 8, None, 4, 1.0, 0, None, None, 0, None) == -1
    assert b'dtype' in L.fewbit_hipx_last_error()
    assert L.fewbit_hipx_sampled_dft(2, None, 1024, 8, 8, None, 4, 1.0, 1, None, None, 0, None) == -1
    assert b'out_dtype' in L.fewbit_hipx_last_error()
    assert L.fewbit_hipx_sampled_dft_seeded(0, None, 3000, 8, 8, 1, None, 4, 1.0, 0, None, None, 0, None) == -2
    assert b'rows = 3000' in L.fewbit_hipx_last_error()
    assert L.fewbit_hipx_sampled_dft_seeded(0, None, 1024, 8, 8, 1, 12, 4, 1.0, 0, None, None, 0, None) == -1
    assert b'8-byte aligned' in L.fewbit_hipx_last_error()
    # proj = 0: nothing to do, whatever the rows
    assert L.fewbit_hipx_sampled_dft(0, None, 3000, 8, 8, None, 0, 1.0, 0, None, None, 0, None) == 0


def test_the_layer_asks_the_library_of_each_kind_which_row_counts_have_a_kernel():
    """linear's row predicate for 'dct' / 'dft' is "that library's workspace query is non-zero": every supported row count, its neighbours,
    7 x 2^k, 0 and counts past 262144; a 'dct' question does not load the companion library"""
    from fewbit_amd import linear
    sweep = sorted({0, 1, 262145, 393216, 524288, 1 << 20} | {r + d for r in SUPPORTED for d in (-1, 0, 1)} | {7 << k for k in range(16)})
    for kind, workspace in (('dct', cabi.sampled_dct_workspace_bytes), ('dft', cabi_x.sampled_dft_workspace_bytes)):
        assert all(linear._transform_rows(kind, rows) for rows in SUPPORTED), kind
        for rows in sweep:
            assert linear._transform_rows(kind, rows) == (workspace(rows, 1, 1) != 0), (kind, rows)
    code = ('import sys; sys.path.insert(0, %r)\n'
            'from fewbit_amd import cabi_x, linear\n'
            'assert linear._transform_rows("dct", 16384) and not linear._transform_rows("dct", 3000) and cabi_x._lib is None' % str(ROOT))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
