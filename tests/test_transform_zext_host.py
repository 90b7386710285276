"""The zero-extended sampled transforms without a GPU: the ceiling of a row count, the exported symbols, the refusals, the switch of the
layer (off by default), and the estimator itself -- mean and variance of (S G)^T (S X), S = sqrt(N' / p) R C' P, in float64 on the host."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.fft
import torch

from fewbit_amd import cabi, cabi_x, linear
from helpers import ROOT

ZEXT_SYMBOLS = ('fewbit_hipx_sampled_rows_ceil', 'fewbit_hipx_sampled_dct_zext', 'fewbit_hipx_sampled_dct_zext_seeded', 'fewbit_hipx_sampled_dft_zext',
                'fewbit_hipx_sampled_dft_zext_seeded')


def test_the_ceiling_is_the_least_supported_row_count_for_every_row_count():
    """against a brute-force minimum over the workspace query (the library's own statement of which row counts have a kernel)"""
    L = cabi_x.lib()
    top = 262145
    supported = np.array([L.fewbit_hipx_sampled_dft_workspace(0, r, 1, 1) != 0 for r in range(top + 1)])
    assert supported.sum() == 11 + 7 + 6 + 5 + 5 + 4
    counts = np.flatnonzero(supported)
    want = np.zeros(top + 1, dtype=np.int64)
    at = np.searchsorted(counts, np.arange(top + 1), side='left')
    inside = at < len(counts)
    want[inside] = counts[at[inside]]
    want[0] = 0
    got = np.array([L.fewbit_hipx_sampled_rows_ceil(r) for r in range(top + 1)], dtype=np.int64)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:10], got[bad[:10]], want[bad[:10]])
    assert cabi_x.sampled_rows_ceil(0) == 0 and cabi_x.sampled_rows_ceil(1 << 40) == 0
    with pytest.raises(cabi.FewbitHipError):
        cabi_x.sampled_rows_ceil(-1)


def test_spot_values_of_the_ceiling():
    """(257 -> 512: 512 = 2^9 has a kernel and is the least count >= 257, as the brute-force test above confirms; a list that names 768 for
    it contradicts the definition "the smallest supported count >= rows")"""
    for rows, want in ((1, 256), (256, 256), (257, 512), (1792, 2048), (3000, 3072), (2100, 2304), (3700, 3840), (12800, 14336), (51200, 57344),
                       (57345, 65536), (81920, 131072), (262144, 262144), (262145, 0)):
        assert cabi_x.sampled_rows_ceil(rows) == want, rows
    # consecutive supported counts: at most a factor 1.25 apart inside 2048 .. 57344 (below: 256, 512, 768, ... 1536, 2048), at most 2 up to 2^18
    counts = sorted({cabi_x.sampled_rows_ceil(r) for r in range(1, 262145, 64)} | {256})
    for a, b in zip(counts, counts[1:]):
        assert b <= (1.25 if 2048 <= a and b <= 57344 else 2) * a, (a, b)


def test_the_header_declares_exactly_what_the_library_exports_and_the_versions_stand():
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    declared = sorted(set(re.findall(r'\b(fewbit_hipx_\w+)\s*\(', header)))
    out = subprocess.run(['nm', '-D', '--defined-only', str(cabi_x.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert exported == declared == sorted(cabi_x.SYMBOLS)
    assert set(ZEXT_SYMBOLS) <= set(exported)
    assert cabi_x.lib().fewbit_hipx_revision() == cabi_x.REVISION == 2
    assert cabi_x.lib().fewbit_hipx_abi_version() == cabi_x.ABI_VERSION == 1
    assert '#define FEWBIT_HIPX_REVISION 2' in header and '#define FEWBIT_HIPX_ABI_VERSION 1' in header


def test_a_library_without_the_symbols_is_refused_by_name():
    code = ('import os, sys; sys.path.insert(0, %r)\n'
            'os.environ["FEWBIT_HIPX_LIB"] = %r\n'
            'from fewbit_amd import cabi_x, cabi\n'
            'try:\n    cabi_x.lib()\nexcept cabi.FewbitHipError as e:\n    assert "fewbit_hipx_sampled_dct_zext" in str(e) and "fewbit_hipx_sampled_rows_ceil" in str(e), e\n'
            'else:\n    raise SystemExit("loaded")' % (str(ROOT), str(cabi.LIB_PATH)))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_calls_are_refused_by_name_before_anything_is_launched():
    L = cabi_x.lib()
    err = L.fewbit_hipx_last_error
    dct, dcts, dft, dfts = L.fewbit_hipx_sampled_dct_zext, L.fewbit_hipx_sampled_dct_zext_seeded, L.fewbit_hipx_sampled_dft_zext, L.fewbit_hipx_sampled_dft_zext_seeded
    # rows without a kernel
    assert dct(0, 16, 3000, 10, 8, 8, 16, 4, 1.0, 16, 16, 1 << 30, None) == -2 and b'rows = 3000' in err() and b'sampled_dct_zext' in err()
    assert dfts(0, 16, 300, 10, 8, 8, 1, None, 4, 1.0, 0, 16, 16, 1 << 30, None) == -2 and b'rows = 300' in err() and b'sampled_dft_zext' in err()
    # valid_rows = 0 or beyond rows
    for valid in (0, 3073, 1 << 40):
        assert dct(0, 16, 3072, valid, 8, 8, 16, 4, 1.0, 16, 16, 1 << 30, None) == -1 and b'valid_rows' in err()
        assert dcts(1, 16, 3072, valid, 8, 8, 1, None, 4, 1.0, 16, 16, 1 << 30, None) == -1 and b'valid_rows' in err()
        assert dft(2, 16, 3072, valid, 8, 8, 16, 4, 1.0, 2, 16, 16, 1 << 30, None) == -1 and b'valid_rows' in err()
        assert dfts(0, 16, 3072, valid, 8, 8, 1, None, 4, 1.0, 0, 16, 16, 1 << 30, None) == -1 and b'valid_rows' in err()
    # an unknown dtype; an out_dtype that is neither F32 nor the input's
    assert dct(9, 16, 3072, 3000, 8, 8, 16, 4, 1.0, 16, 16, 1 << 30, None) == -1 and b'dtype' in err()
    assert dft(9, 16, 3072, 3000, 8, 8, 16, 4, 1.0, 0, 16, 16, 1 << 30, None) == -1 and b'dtype' in err()
    assert dft(2, 16, 3072, 3000, 8, 8, 16, 4, 1.0, 1, 16, 16, 1 << 30, None) == -1 and b'out_dtype' in err()
    # a short, a missing and a misaligned workspace (the formula at `rows`)
    need = cabi_x.sampled_dft_workspace_bytes(3072, 8, 4, torch.float32)
    assert need == 3072 * 256 + 2048 + 32
    assert dct(0, 16, 3072, 3000, 8, 8, 16, 4, 1.0, 16, 16, need - 1, None) == -1 and b'workspace' in err()
    assert dfts(0, 16, 3072, 3000, 8, 8, 1, None, 4, 1.0, 0, 16, None, 0, None) == -1 and b'workspace' in err()
    assert dft(0, 16, 3072, 3000, 8, 8, 16, 4, 1.0, 0, 16, 24, need + 64, None) == -1 and b'aligned' in err()
    # null pointers, a leading dimension below the features, a misaligned seed word, a matrix of 4 GiB or more
    assert dct(0, None, 3072, 3000, 8, 8, 16, 4, 1.0, 16, 16, need, None) == -1 and b'null' in err()
    assert dct(0, 16, 3072, 3000, 8, 7, 16, 4, 1.0, 16, 16, need, None) == -1 and b'leading dimension' in err()
    assert dfts(0, 16, 3072, 3000, 8, 8, 1, 12, 4, 1.0, 0, 16, 16, need, None) == -1 and b'8-byte aligned' in err()
    assert dct(0, 16, 3072, 3000, 8, 1 << 20, 16, 4, 1.0, 16, 16, need, None) == -2 and b'4 GiB' in err()
    # nothing to do: no samples
    assert dct(0, None, 3000, 0, 8, 8, None, 0, 1.0, None, None, 0, None) == 0


def test_the_switch_is_off_by_default_and_returns_its_previous_value():
    assert 'FEWBIT_EXTEND_ROWS' not in os.environ or os.environ['FEWBIT_EXTEND_ROWS'] in ('0', '')
    assert linear.use_row_extension() is False
    x = torch.zeros(3000, 8)
    torch_fft = 'torch.fft (rocFFT on the GPU): full transform along dim 0 in fp32, then the gather of the sampled rows'
    for kind in ('dct', 'dft'):
        assert linear.sampled_transform_path(kind, x) == torch_fft
        for rows in (3000, 1792, 640, 100, 81920):
            assert not linear._transform_rows(kind, rows)
    assert linear.use_row_extension(True) is False
    try:
        assert linear.use_row_extension() is True
        assert not linear._transform_rows('dct', 3000)                  # (which row counts have a kernel does not depend on the switch)
        assert linear.sampled_transform_path('dct', x) == torch_fft     # (a host tensor keeps torch.fft)
        assert linear.use_row_extension(False) is True
    finally:
        linear.use_row_extension(False)
    assert linear.use_row_extension() is False


def test_a_matrix_of_4_gib_or_more_is_outside_the_zero_extended_path():
    """the bound of fewbit_fft4.h::zext_span_ok (the C entry points refuse beyond it, above): rows x ld x itemsize <= 0xfffffff0"""
    assert linear._zext_span_ok(3000, 40, 4) and linear._zext_span_ok(0xfffffff0 // 16, 8, 2) and linear._zext_span_ok(0xfffffff0 // 4, 1, 4)
    assert not linear._zext_span_ok(0xfffffff0 // 16 + 1, 8, 2) and not linear._zext_span_ok(200000, 11008, 2) and not linear._zext_span_ok(250000, 4608, 4)
    L = cabi_x.lib()
    need = cabi_x.sampled_dft_workspace_bytes(262144, 8, 4, torch.float32)
    assert linear._zext_span_ok(262144, 8191, 2) and not linear._zext_span_ok(262144, 8192, 2)
    # the largest span the C entry point takes is the largest the layer routes to it (that call is then refused for its short workspace)
    assert L.fewbit_hipx_sampled_dct_zext(1, 16, 262144, 262144, 8, 8191, 16, 4, 1.0, 16, 16, need - 1, None) == -1 and b'workspace' in L.fewbit_hipx_last_error()
    assert L.fewbit_hipx_sampled_dct_zext(1, 16, 262144, 262144, 8, 8192, 16, 4, 1.0, 16, 16, need, None) == -2 and b'4 GiB' in L.fewbit_hipx_last_error()


def test_the_environment_variable_sets_the_switch_in_a_child_process():
    for value, want in (('1', True), ('0', False), (None, False)):
        env = {k: v for k, v in os.environ.items() if k != 'FEWBIT_EXTEND_ROWS'}
        if value is not None:
            env['FEWBIT_EXTEND_ROWS'] = value
        code = 'import sys; sys.path.insert(0, %r)\nfrom fewbit_amd import linear\nprint(linear.use_row_extension())' % str(ROOT)
        r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and r.stdout.strip() == str(want), (value, r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize('big', (768, 512))
def test_the_zero_extended_estimator_is_unbiased_and_has_the_closed_form_variance(big):
    """N = 300 at N' = 768 (any supported N' >= N gives an estimator of this kind) and at N' = 512, the ceiling of 300 and what the layer
    runs; 6 x 5 features, p = 60, white Gaussian X and G, rows of cabi.sampled_rows(seed, N', p).  Per draw the estimate is
    (N' / p) sum_j (u_kj^T G)^T (u_kj^T X), u_k the rows of C' P.  Over D draws: the mean is within 5 standard errors of G^T X per entry, and
    the mean squared deviation ||estimate - G^T X||_F^2 within 5 standard errors of (N' sum_k ||u_k^T X||^2 ||u_k^T G||^2 - ||X^T G||_F^2) / p;
    the standard errors are those of the draws themselves."""
    n, f_in, f_out, p, draws = 300, 6, 5, 60, 4000
    assert cabi_x.sampled_dft_workspace_bytes(big, 1, 1) != 0 and cabi_x.sampled_rows_ceil(n) == 512
    rng = np.random.default_rng(20261017)
    x, g = rng.standard_normal((n, f_in)), rng.standard_normal((n, f_out))
    pad = lambda m: np.concatenate([m, np.zeros((big - n, m.shape[1]))])
    tx, tg = scipy.fft.dct(pad(x), axis=0, norm='ortho'), scipy.fft.dct(pad(g), axis=0, norm='ortho')       # rows k: u_k^T X, u_k^T G
    exact = g.T @ x
    estimates = np.empty((draws, f_out, f_in))
    for d in range(draws):
        k = cabi.sampled_rows(1000 + d, big, p).numpy()
        estimates[d] = (big / p) * tg[k].T @ tx[k]
    mean, sem = estimates.mean(0), estimates.std(0, ddof=1) / np.sqrt(draws)
    worst = float(np.abs((mean - exact) / sem).max())
    print(f"N' = {big}: mean: worst deviation {worst:.2f} standard errors over {exact.size} entries")
    assert worst <= 5.0
    msd = ((estimates - exact)**2).sum((1, 2))
    closed = (big * ((tx**2).sum(1) * (tg**2).sum(1)).sum() - (exact**2).sum()) / p
    z = (msd.mean() - closed) / (msd.std(ddof=1) / np.sqrt(draws))
    # the exact-length estimator (the reference's dct(X)[idx] at length N, scale N / p): its closed form, for the record (not asserted)
    ex, eg = scipy.fft.dct(x, axis=0, norm='ortho'), scipy.fft.dct(g, axis=0, norm='ortho')
    closed_exact = (n * ((ex**2).sum(1) * (eg**2).sum(1)).sum() - (exact**2).sum()) / p
    print(f'mean squared deviation {msd.mean():.2f}, closed form {closed:.2f} ({z:+.2f} standard errors); exact-length closed form {closed_exact:.2f}; '
          f'ratio zero-extended / exact-length {closed / closed_exact:.4f}')
    assert abs(z) <= 5.0
