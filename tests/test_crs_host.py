"""The columns of a seed (include/fewbit_hipx.h, "The columns of a seed") without a GPU: fewbit_hipx_crs_columns against a restatement of the
definition built on the FROZEN library's Philox (fewbit_hip_philox4x32), the uniformity of the draws, and the surface of the new entry
points of libfewbit_hipx.so (workspace query, revision, symbol list)."""
import math
import re

import numpy as np
import pytest
import torch

from fewbit_amd import cabi, cabi_x
from helpers import ROOT

COLS_DOMAIN = 4                     # counter word 3 of the column draws (0, 2: the dense sketches; 3: the sampled rows)


def columns_of_seed(seed, in_features, nopairs):
    """the definition, restated: -> (ascending distinct columns, their counts, their fp32 scales)"""
    key = (seed & 0xffffffff, (seed >> 32) & 0xffffffff)
    count = {}
    for q in range(-(-nopairs // 4)):
        words = cabi.philox4x32((q, 0, 0, COLS_DOMAIN), key)
        for h in range(min(4, nopairs - 4 * q)):
            col = (words[h] * in_features) >> 32
            count[col] = count.get(col, 0) + 1
    cols = sorted(count)
    return cols, [count[c] for c in cols], [np.float32(count[c] * in_features / nopairs) for c in cols]


@pytest.mark.parametrize('in_features', (1, 7, 768, 3072, 16384))
def test_the_host_function_is_the_definition(in_features):
    for nopairs in sorted({1, 5, max(in_features // 2, 1), 4 * in_features}):
        for seed in (0, 1, 0x5eed5eed5eed, 2**62 - 1, 0xfedcba9876543210):
            if in_features == 16384 and nopairs > 5 and seed > 1:
                continue                                            # (the Python restatement is slow: two seeds at the big shapes)
            cols, count = cabi_x.crs_columns(seed, in_features, nopairs)
            want_cols, want_count, _ = columns_of_seed(seed, in_features, nopairs)
            assert cols.dtype == torch.int64 and count.dtype == torch.int32
            assert cols.tolist() == want_cols and count.tolist() == want_count, (seed, in_features, nopairs)
            assert all(a < b for a, b in zip(want_cols, want_cols[1:])) and 0 <= cols.min() and cols.max() < in_features
            assert int(count.min()) >= 1 and int(count.sum()) == nopairs
            assert cabi_x.crs_count(seed, in_features, nopairs) == len(want_cols) <= min(nopairs, in_features)


@pytest.mark.parametrize('in_features', (1023, 1025, 8191, 8193))
def test_the_host_function_is_the_definition_around_the_prep_kernels_boundaries(in_features):
    """the widths on either side of the prep kernel's 1024 threads and of its 8192 LDS counters, at one draw and at one draw past a full
    pass of its draw loop (4 x 1024 + 1): what tests/test_gpu_crs_edges.py holds the device's evaluation against"""
    for nopairs in (1, 4097):
        for seed in (1, 0xfedcba9876543210):
            cols, count = cabi_x.crs_columns(seed, in_features, nopairs)
            want_cols, want_count, want_scale = columns_of_seed(seed, in_features, nopairs)
            assert cols.tolist() == want_cols and count.tolist() == want_count, (seed, in_features, nopairs)
            assert int(count.sum()) == nopairs and cabi_x.crs_count(seed, in_features, nopairs) == len(want_cols) <= min(nopairs, in_features)
            scale = (count.double() * in_features / nopairs).float()
            assert scale.tolist() == [float(s) for s in want_scale]


def test_the_column_domain_is_not_the_rows_or_a_sketch_domain():
    """one seed used for a sketch, for sampled rows and for columns: three different Philox blocks"""
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    assert re.search(r'counter = \(q, 0, 0, 4\)', header)
    key = (123, 456)
    blocks = {d: cabi.philox4x32((0, 0, 0, d), key) for d in (0, 2, 3, COLS_DOMAIN)}
    assert len(set(blocks.values())) == 4
    # 768 = 3 x 2^8 rows draw word x rows >> 32 as well: same formula, other block, other numbers
    rows = cabi.sampled_rows(123 | 456 << 32, 768, 64).tolist()
    draws = [(w * 768) >> 32 for q in range(16) for w in cabi.philox4x32((q, 0, 0, COLS_DOMAIN), key)]
    assert rows != draws


def test_the_draws_are_uniform():
    """2000 seeds, in_features = 64, nopairs = 32: a column is hit by a draw with p = 1 / 64, so its hits over n = 2000 * 32 draws are
    Binomial(n, p): every column within five standard deviations sqrt(n p (1 - p)) of n p (64 columns: a false alarm at ~4e-5)"""
    in_features, nopairs, seeds = 64, 32, 2000
    hits = torch.zeros(in_features, dtype=torch.int64)
    gen = torch.Generator().manual_seed(11)
    for seed in torch.randint(0, 2**62, (seeds, ), generator=gen).tolist():
        cols, count = cabi_x.crs_columns(seed, in_features, nopairs)
        hits[cols] += count.long()
    n, p = seeds * nopairs, 1.0 / in_features
    assert int(hits.sum()) == n
    bound = 5.0 * math.sqrt(n * p * (1.0 - p))
    assert float((hits.double() - n * p).abs().max()) <= bound, (hits.tolist(), n * p, bound)


def test_the_surface_of_the_new_entry_points():
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    # shapes without a kernel have no workspace
    assert cabi_x.crs_workspace_bytes(16, 768, 384, torch.float64) == 0
    assert cabi_x.crs_workspace_bytes(16, 0, 384) == 0 == cabi_x.crs_workspace_bytes(16, 768, 0)
    assert cabi_x.crs_workspace_bytes(0, 768, 384) == 0
    assert cabi_x.lib().fewbit_hipx_crs_workspace(7, 16, 768, 384) == 0                 # (an unknown dtype, at the C level)
    # the range the header states: in_features up to 2^20 (at least 16384), nopairs up to 2^22 (at least 2^20), three dtypes
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        for in_features, nopairs in ((1, 1), (770, 385), (16384, 1), (16384, 1 << 20), (1 << 20, 1 << 22)):
            cap = min(in_features, nopairs)
            assert cabi_x.crs_workspace_bytes(1, in_features, nopairs, dtype) == 16 + -(-4 * in_features // 16) * 16 + 2 * (-(-4 * cap // 16) * 16)
    assert cabi_x.crs_workspace_bytes(1, (1 << 20) + 1, 5) == 0 == cabi_x.crs_workspace_bytes(1, 5, (1 << 22) + 1)
    # the revision: the header's, the binding's; the ABI version stays 1
    revision = int(re.search(r'#define FEWBIT_HIPX_REVISION (\d+)', header).group(1))
    assert cabi_x.lib().fewbit_hipx_revision() == revision == cabi_x.REVISION == 2
    assert cabi_x.lib().fewbit_hipx_abi_version() == 1
    declared = sorted(set(re.findall(r'\b(fewbit_hipx_\w+)\s*\(', header)))
    assert declared == sorted(cabi_x.SYMBOLS)
    assert {'fewbit_hipx_crs_columns', 'fewbit_hipx_crs_workspace', 'fewbit_hipx_crs_gather', 'fewbit_hipx_crs_scatter'} <= set(declared)


def test_calls_are_refused_by_name_before_anything_is_launched():
    L = cabi_x.lib()
    assert L.fewbit_hipx_crs_gather(9, None, 4, 8, 8, 1, None, 4, 4, None, None, 0, None) == -1
    assert b'dtype' in L.fewbit_hipx_last_error()
    assert L.fewbit_hipx_crs_gather(0, None, 4, 0, 8, 1, None, 4, 4, None, None, 0, None) == -2
    assert b'in_features = 0' in L.fewbit_hipx_last_error()
    assert L.fewbit_hipx_crs_gather(0, None, 4, 8, 8, 1, None, 4, 5, None, None, 0, None) == -1
    assert b'cap = 5' in L.fewbit_hipx_last_error()
    assert L.fewbit_hipx_crs_scatter(0, None, 4, 4, 1, 12, 8, 4, None, None, 0, None) == -1
    assert b'8-byte aligned' in L.fewbit_hipx_last_error()
    assert L.fewbit_hipx_crs_scatter(0, None, 4, 4, 1, None, 8, 4, None, None, 0, None) == -1
    assert b'workspace' in L.fewbit_hipx_last_error()
    assert L.fewbit_hipx_crs_columns(1, 8, 0, None, None, None) == -2
    assert b'nopairs = 0' in L.fewbit_hipx_last_error()


def test_a_library_without_the_new_symbols_is_refused_by_name(monkeypatch):
    """cabi_x.lib() on a library that lacks an entry point of SYMBOLS (here: the frozen library, which has none of them) names what is missing"""
    monkeypatch.setattr(cabi_x, '_lib', None)
    monkeypatch.setattr(cabi_x, 'LIB_PATH', cabi.LIB_PATH)
    with pytest.raises(cabi.FewbitHipError, match='lacks .*fewbit_hipx_crs_gather'):
        cabi_x.lib()
    monkeypatch.undo()
    assert cabi_x.lib().fewbit_hipx_revision() == 2
