"""The moments of the variance estimator without a GPU: the three entry points of the companion library (exported, declared, refused by
name when a library lacks them), their refusals before anything is launched, and ``fewbit_amd.variance`` on host tensors --
``gradient_moments`` against the golden values of the reference's formulas, ``VarianceEstimator`` against the fp32 formulation it replaced."""
import ctypes
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import fewbit_amd as fewbit
from fewbit_amd import cabi, cabi_x, variance
from fewbit_amd.linear import LinearGRP

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / 'tests' / 'golden'
MOMENT_SYMBOLS = ('fewbit_hipx_moments_workspace', 'fewbit_hipx_row_moments', 'fewbit_hipx_sum_squares')
WORKSPACE = 1024 * 3 * 8                          # kMaxGroups partials of three doubles (fewbit_moments.hip)


def test_the_three_symbols_are_exported_declared_and_bound():
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    declared = set(re.findall(r'\b(fewbit_hipx_\w+)\s*\(', header))
    out = subprocess.run(['nm', '-D', '--defined-only', str(cabi_x.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in MOMENT_SYMBOLS:
        assert name in declared and name in exported and name in cabi_x.SYMBOLS, name
    assert cabi_x.lib().fewbit_hipx_revision() == cabi_x.REVISION == 2 and cabi_x.lib().fewbit_hipx_abi_version() == cabi_x.ABI_VERSION == 1
    assert 'fewbit_hipx_moments_workspace, _row_moments, _sum_squares' in header          # the version history says where they live


def test_a_library_without_the_symbols_is_refused_by_name(monkeypatch):
    monkeypatch.setattr(cabi_x, '_lib', None)
    monkeypatch.setattr(cabi_x, 'LIB_PATH', cabi.LIB_PATH)          # the frozen library has none of them
    with pytest.raises(cabi.FewbitHipError) as e:
        cabi_x.lib()
    for name in MOMENT_SYMBOLS:
        assert name in str(e.value)
    monkeypatch.undo()
    assert cabi_x.lib().fewbit_hipx_revision() == 2


def test_the_workspace_query():
    assert cabi_x.moments_workspace_bytes(16384, 768, 3072) == WORKSPACE
    assert cabi_x.moments_workspace_bytes(1, 1, 1) == WORKSPACE and cabi_x.moments_workspace_bytes(770 * 3072) == WORKSPACE
    assert cabi_x.moments_workspace_bytes(2**31, 2**24, 2**24) == WORKSPACE
    for rows, n, m in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (2**31 + 1, 8, 8), (8, 2**24 + 1, 8), (8, 8, 2**24 + 1), (-1, 8, 8)):
        assert cabi_x.moments_workspace_bytes(rows, n, m) == 0, (rows, n, m)


def test_calls_are_refused_by_code_and_text_before_anything_is_launched():
    """(null and fake pointers throughout: a call that got as far as a launch would fail loudly)"""
    L = cabi_x.lib()
    err = lambda: L.fewbit_hipx_last_error().decode()
    rm, ss = L.fewbit_hipx_row_moments, L.fewbit_hipx_sum_squares
    fake = 4096                                                       # an aligned non-null address that is never dereferenced
    # unknown dtypes: -1
    assert rm(3, fake, 8, 8, 0, fake, 8, 8, 4, fake, fake, WORKSPACE, None) == -1 and 'dtype_x 3' in err()
    assert rm(0, fake, 8, 8, -1, fake, 8, 8, 4, fake, fake, WORKSPACE, None) == -1 and 'dtype_g -1' in err()
    assert ss(7, fake, 8, fake, fake, WORKSPACE, None) == -1 and 'dtype 7' in err()
    # unsupported sizes: -2, the offending value named
    assert rm(0, fake, 8, 8, 0, fake, 8, 8, 0, fake, fake, WORKSPACE, None) == -2 and 'rows = 0' in err()
    assert rm(0, fake, 0, 8, 0, fake, 8, 8, 4, fake, fake, WORKSPACE, None) == -2 and 'n = 0' in err()
    assert rm(0, fake, 8, 8, 0, fake, 0, 8, 4, fake, fake, WORKSPACE, None) == -2 and 'm = 0' in err()
    assert rm(0, fake, 8, 7, 0, fake, 8, 8, 4, fake, fake, WORKSPACE, None) == -2 and 'ldx = 7 < n = 8' in err()
    assert rm(0, fake, 8, 8, 0, fake, 9, 8, 4, fake, fake, WORKSPACE, None) == -2 and 'ldg = 8 < m = 9' in err()
    assert rm(0, fake, 8, 8, 0, fake, 8, 8, 2**31 + 1, fake, fake, WORKSPACE, None) == -2 and f'rows = {2**31 + 1}' in err()
    assert rm(0, fake, 2**24 + 1, 2**24 + 1, 0, fake, 8, 8, 4, fake, fake, WORKSPACE, None) == -2 and f'n = {2**24 + 1}' in err()
    assert rm(0, fake, 8, 8, 0, fake, 2**24 + 1, 2**24 + 1, 4, fake, fake, WORKSPACE, None) == -2 and f'm = {2**24 + 1}' in err()
    assert rm(0, fake, 8, 2**31 + 1, 0, fake, 8, 8, 4, fake, fake, WORKSPACE, None) == -2 and f'ldx = {2**31 + 1}' in err()
    assert ss(0, fake, 0, fake, fake, WORKSPACE, None) == -2 and 'count = 0' in err()
    assert ss(0, fake, 2**31 + 1, fake, fake, WORKSPACE, None) == -2 and f'count = {2**31 + 1}' in err()
    # a short, missing or misaligned workspace: -1 with "workspace" in the text
    assert rm(0, fake, 8, 8, 2, fake, 8, 8, 4, fake, fake, WORKSPACE - 1, None) == -1 and 'workspace' in err() and str(WORKSPACE) in err()
    assert rm(0, fake, 8, 8, 2, fake, 8, 8, 4, fake, None, 0, None) == -1 and 'workspace' in err()
    assert rm(0, fake, 8, 8, 2, fake, 8, 8, 4, fake, fake + 8, WORKSPACE, None) == -1 and 'workspace' in err()
    assert ss(1, fake, 8, fake, fake, 16, None) == -1 and 'workspace' in err()
    # null and misaligned operands: -1
    assert rm(0, None, 8, 8, 0, fake, 8, 8, 4, fake, fake, WORKSPACE, None) == -1 and 'null' in err()
    assert rm(0, fake + 2, 8, 8, 1, fake, 8, 8, 4, fake, fake, WORKSPACE, None) == -1 and 'aligned' in err()
    assert ss(2, fake + 1, 8, fake, fake, WORKSPACE, None) == -1 and 'aligned' in err()
    assert ss(2, fake, 8, None, fake, WORKSPACE, None) == -1 and 'null' in err()


def test_the_bindings_refuse_host_tensors_and_mismatched_rows():
    with pytest.raises(cabi.FewbitHipError, match='GPU'):
        cabi_x.row_moments(torch.zeros(4, 3), torch.zeros(4, 5))
    with pytest.raises(cabi.FewbitHipError, match='GPU'):
        cabi_x.sum_squares(torch.zeros(4))
    with pytest.raises(cabi.FewbitHipError, match='2-D'):
        cabi_x.row_moments(torch.zeros(4), torch.zeros(4, 5))


# ---- fewbit_amd.variance on the host -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lref():
    with np.load(GOLDEN / 'linear_ref.npz') as z:
        return {k: z[k].copy() for k in z.files}


def _formulas(moments, bs, bs_proj):
    sx, sg, sxg, cross = moments.unbind(0)
    return cross / (sx * sg), sxg * (bs / (bs - 1)) - cross / (bs - 1), (sx * sg - cross) / bs_proj


def test_gradient_moments_on_float64_host_tensors_reproduces_the_golden_values(lref):
    a, b = torch.from_numpy(lref['var_input']), torch.from_numpy(lref['var_output'])
    assert a.dtype == torch.float64
    moments = variance.gradient_moments(a, b)
    assert moments.shape == (4, ) and moments.dtype == torch.float64 and moments.device == a.device
    rows = a.shape[0]
    corr, var_sgd, var_rmm = _formulas(moments, rows, rows)
    for got, key in ((corr, 'var_correlation'), (var_sgd, 'var_sgd'), (_formulas(moments, 12, 5)[1], 'var_sgd_bs12'), (var_rmm, 'var_rmm'),
                     (_formulas(moments, 12, 5)[2], 'var_rmm_bs5')):
        assert torch.allclose(got, torch.from_numpy(lref[key]), rtol=1e-12, atol=0), key
    # leading dimensions are flattened, and the definitions are what they say
    again = variance.gradient_moments(a.reshape(2, -1, a.shape[1]), b.reshape(2, -1, b.shape[1]))
    assert torch.equal(again, moments)
    want = torch.stack(((a * a).sum(), (b * b).sum(), ((a * a).sum(1) * (b * b).sum(1)).sum(), ((a.T @ b)**2).sum()))
    assert torch.allclose(moments, want, rtol=1e-13, atol=0)
    assert 'float64 PyTorch' in variance.variance_path(a, b)


@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16, torch.float64))
def test_the_estimator_on_the_host_gives_what_the_fp32_formulation_gave(dtype, monkeypatch):
    """Before: ``.float()`` copies and the three ``estimate_*`` functions in fp32.  Now: float64 moments, rounded once to fp32.  The two agree to
    the error of the fp32 formulation: a handful of roundings of 2^-24 on sums of <= 40 x 8 positive terms, relative to sx sg for the
    differences of var_sgd and var_rmm (both subtract cross from a larger product)."""
    torch.manual_seed(11)
    calls = []
    real = variance._cross_product
    monkeypatch.setattr(variance, '_cross_product', lambda x, g: calls.append(1) or real(x, g))
    seen = []
    est = fewbit.variance.VarianceEstimator(LinearGRP(8, 4, proj_dim=5).to(dtype), lambda *a: seen.append(a))
    inp = torch.randn(40, 8).to(dtype)
    est(inp).square().sum().backward()
    assert len(calls) <= 1                                           # (host tensors do not take the GEMM seam at all)
    corr, var_sgd, var_rmm = est.variance
    assert len(seen) == 1 and seen[0][3] == 0 and est.state.step == 1 and all(s is v for s, v in zip(seen[0][:3], est.variance))
    x, g = est.state.input.float(), est.state.grad_output.float()
    assert torch.equal(est.state.input, inp) and est.state.grad_output.shape == (40, 4)
    scale = float(torch.linalg.norm(x)**2 * torch.linalg.norm(g)**2)
    for got, want, slack in ((corr, variance.estimate_correlation(x, g), 1.0), (var_sgd, variance.estimate_variance_sgd(x, g, 40), scale / 39),
                             (var_rmm, variance.estimate_variance_rmm(x, g, 5), scale / 5)):
        assert got.dtype == torch.float32 and got.dim() == 0
        assert abs(float(got) - float(want)) <= 64 * 2.0**-24 * slack, (float(got), float(want))


def test_postprocess_calls_the_gemm_seam_at_most_once_and_one_row_raises_as_before(monkeypatch):
    calls = []
    monkeypatch.setattr(variance, '_cross_product', lambda x, g: calls.append(1) or (g.T.float() @ x.float()))
    state = variance._VarianceState()
    state.postprocess()                                              # nothing stored yet: a no-op
    assert state.variance is None and state.step == 0
    state.bs, state.bs_proj = 6, 3
    state.forward(torch.arange(12.0).reshape(6, 2))
    state.backward(torch.ones(6, 3))
    assert len(calls) <= 1 and state.step == 1
    sx, sg = float((torch.arange(12.0)**2).sum()), 18.0
    cross = 3 * float((torch.arange(12.0).reshape(6, 2).sum(0)**2).sum())
    assert float(state.variance[2]) == pytest.approx((sx * sg - cross) / 3, rel=1e-6)
    # one row: B - 1 = 0 divides by zero on the host, as it always has
    one = variance._VarianceState()
    one.bs, one.bs_proj = 1, 1
    one.forward(torch.ones(1, 2))
    with pytest.raises(ZeroDivisionError):
        one.backward(torch.ones(1, 3))
