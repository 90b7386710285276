"""The dropout of a seed without a GPU: the three entry points of the companion library (declared, exported, bound, refused by name when a
library lacks them), the mask of a seed against its known answers, against an independent restatement through the frozen library's Philox
and against its binomial statistics, the refusals before anything is launched, and ``fewbit_amd.dropout`` on host tensors."""
import importlib
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fewbit_amd as fewbit
from fewbit_amd import cabi, cabi_x

ROOT = Path(__file__).resolve().parents[1]
DROPOUT_SYMBOLS = ('fewbit_hipx_dropout_threshold', 'fewbit_hipx_dropout_keep', 'fewbit_hipx_dropout')
ONE = 65536
GOLDEN_SEED = 0x9E3779B97F4A7C15
# (seed, first element): u of the eight elements from there -- from a numpy model of the definition in include/fewbit_hipx.h
KNOWN_U = {
    (1234, 0): (64538, 60214, 57172, 61639, 41034, 26606, 24601, 57880),
    (1234, 8): (12631, 9826, 31752, 2194, 2245, 22311, 31230, 18346),
    (1234, 2**35): (6484, 37029, 51781, 44792, 64130, 27134, 36500, 13430),           # counter word 1 = 1
    (GOLDEN_SEED, 0): (65506, 1362, 29401, 12679, 51404, 424, 60641, 15407),
}
KNOWN_DROPS = {(1234, 0.1): 105331, (1234, 0.5): 524232, (1234, 0.9): 943514, (7, 0.1): 104493, (7, 0.5): 524997, (7, 0.9): 943512}
N_STAT = 2**20


def _keep(seed, n, threshold, first=0):
    return cabi_x.dropout_keep(seed, n, threshold / ONE, first)


def test_the_three_symbols_are_exported_declared_and_bound():
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    declared = set(re.findall(r'\b(fewbit_hipx_\w+)\s*\(', header))
    out = subprocess.run(['nm', '-D', '--defined-only', str(cabi_x.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DROPOUT_SYMBOLS:
        assert name in declared and name in exported and name in cabi_x.SYMBOLS, name
    assert cabi_x.lib().fewbit_hipx_revision() == cabi_x.REVISION == 2 and cabi_x.lib().fewbit_hipx_abi_version() == cabi_x.ABI_VERSION == 1
    assert 'fewbit_hipx_dropout_threshold, _dropout_keep, _dropout' in header             # the version history says where they live


def test_a_library_without_the_symbols_is_refused_by_name(monkeypatch):
    monkeypatch.setattr(cabi_x, '_lib', None)
    monkeypatch.setattr(cabi_x, 'LIB_PATH', cabi.LIB_PATH)          # the frozen library has none of them
    with pytest.raises(cabi.FewbitHipError) as e:
        cabi_x.lib()
    for name in DROPOUT_SYMBOLS:
        assert name in str(e.value)
    monkeypatch.undo()
    assert cabi_x.lib().fewbit_hipx_revision() == 2


def test_the_threshold_of_a_probability():
    assert cabi_x.dropout_threshold(0.1) == 6554 and cabi_x.dropout_threshold(0.5) == 32768
    assert cabi_x.dropout_threshold(0) == 0 and cabi_x.dropout_threshold(1) == ONE
    assert cabi_x.dropout_threshold(0.5 / ONE) == 0 and cabi_x.dropout_threshold(1.5 / ONE) == 2          # ties go to the even neighbour
    for t in (1, 6554, 65535):
        assert cabi_x.dropout_threshold(t / ONE) == t
    for p in (-0.1, 1.1, float('nan')):
        assert cabi_x.lib().fewbit_hipx_dropout_threshold(p) == -1
        with pytest.raises(cabi.FewbitHipError, match='between 0 and 1'):
            cabi_x.dropout_threshold(p)
    assert np.float32(65536.0 / (ONE - 6554)) == np.float32(1.1111187)


@pytest.mark.parametrize('seed,first', sorted(KNOWN_U))
def test_known_answers_of_u(seed, first):
    """keep(i) = u(i) >= T: kept at T = u, dropped at T = u + 1 -- which pins u"""
    want = KNOWN_U[(seed, first)]
    for j, u in enumerate(want):
        assert bool(_keep(seed, 1, u, first + j)[0]) and not bool(_keep(seed, 1, u + 1, first + j)[0]), (seed, first, j)
    # and by bisection over T from one call per threshold on all eight
    lo, hi = np.zeros(8, dtype=np.int64), np.full(8, ONE, dtype=np.int64)                 # kept at lo, dropped at hi
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        kept = np.array([bool(_keep(seed, 8, int(mid[j]), first)[j]) for j in range(8)])
        lo, hi = np.where(kept, mid, lo), np.where(kept, hi, mid)
    assert tuple(lo) == want


@pytest.fixture(scope='module')
def masks():
    return {(seed, p): _keep(seed, N_STAT, cabi_x.dropout_threshold(p)).numpy() for seed, p in KNOWN_DROPS}


def test_known_drop_counts(masks):
    for key, want in KNOWN_DROPS.items():
        assert int((~masks[key]).sum()) == want, key


def _restated(seed, first, count, threshold):
    """the definition through the frozen library's Philox"""
    key = (seed & 0xffffffff, seed >> 32)
    out = []
    for i in range(first, first + count):
        q = i >> 3
        w = cabi.philox4x32((q & 0xffffffff, q >> 32, 0, 5), key)
        word = w[(i & 7) >> 1]
        u = (word >> 16) if i & 1 else (word & 0xffff)
        out.append(u >= threshold)
    return torch.tensor(out)


def test_the_random123_known_answer_of_the_frozen_philox():
    assert cabi.philox4x32((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)


@pytest.mark.parametrize('first', (0, 8, 24, 2**35 - 24, 3, 2**32 * 8 - 5))
@pytest.mark.parametrize('seed', (1234, GOLDEN_SEED))
def test_keep_equals_the_definition_restated(seed, first):
    """(count = 100 from 2^35 - 24: the carry into counter word 1 falls inside the call; the odd firsts: the host function takes any)"""
    for threshold in (6554, 32768):
        assert torch.equal(_keep(seed, 100, threshold, first), _restated(seed, first, 100, threshold)), (seed, first, threshold)
    assert bool(_keep(seed, 100, 0, first).all()) and not bool(_keep(seed, 100, ONE, first).any())


@pytest.mark.parametrize('seed,p', sorted(KNOWN_DROPS))
def test_statistics_of_the_mask(masks, seed, p):
    """Deterministic (the seeds are fixed).  With q = T / 65536 and independent elements: the drop count is Binomial(n, q), each of the eight
    positions i & 7 Binomial(n / 8, q), and the lag-1 sum S = sum d_i d_{i+1} over n - 1 pairs has mean (n - 1) q^2 and variance
    (n - 1)(q^2 - q^4) + 2 (n - 2)(q^3 - q^4) (adjacent pairs share one element).  Each within 4 standard deviations."""
    dropped = (~masks[(seed, p)]).astype(np.int64)
    n, q = N_STAT, cabi_x.dropout_threshold(p) / ONE
    z = [(dropped.sum() - n * q) / math.sqrt(n * q * (1 - q))]
    for e in range(8):
        z.append((dropped[e::8].sum() - n / 8 * q) / math.sqrt(n / 8 * q * (1 - q)))
    lag = int((dropped[:-1] * dropped[1:]).sum())
    z.append((lag - (n - 1) * q * q) / math.sqrt((n - 1) * (q**2 - q**4) + 2 * (n - 2) * (q**3 - q**4)))
    print(f'seed {seed} p {p}: max |z| = {max(abs(v) for v in z):.2f}')
    assert max(abs(v) for v in z) <= 4.0, z


def test_calls_are_refused_by_code_and_text_before_anything_is_launched():
    """(null and fake pointers throughout: a call that got as far as a launch would fail loudly)"""
    L = cabi_x.lib()
    err = lambda: L.fewbit_hipx_last_error().decode()
    d, k = L.fewbit_hipx_dropout, L.fewbit_hipx_dropout_keep
    fake = 4096                                                       # an aligned non-null address that is never dereferenced
    assert d(3, fake, None, fake, 64, 0, 1, None, 6554, None) == -1 and 'dtype 3' in err()
    assert d(-1, fake, None, fake, 64, 0, 1, None, 6554, None) == -1 and 'dtype -1' in err()
    assert d(0, None, None, fake, 64, 0, 1, None, 6554, None) == -1 and 'null' in err()
    assert d(0, fake, fake, None, 64, 0, 1, None, 6554, None) == -1 and 'null' in err()
    assert d(2, fake, None, fake, 64, 0, 1, None, ONE + 1, None) == -1 and 'threshold = 65537' in err()
    assert d(2, fake, None, fake, 64, 0, 1, fake + 4, 6554, None) == -1 and '8-byte aligned' in err()
    assert d(2, fake, None, fake, 64, 4, 1, None, 6554, None) == -1 and 'first = 4' in err() and 'multiple of 8' in err()
    assert d(1, fake, None, fake, 64, 2**35 + 1, 1, None, 6554, None) == -1 and f'first = {2**35 + 1}' in err()
    assert d(1, fake + 1, None, fake, 64, 0, 1, None, 6554, None) == -1 and 'aligned' in err()
    assert d(0, fake, fake + 2, fake, 64, 0, 1, None, 6554, None) == -1 and 'aligned' in err()
    # n = 0: nothing to do, whatever the pointers
    assert d(0, None, None, None, 0, 0, 1, None, 6554, None) == 0
    assert d(2, fake, fake, fake, 0, 8, 1, fake, ONE, None) == 0
    # the host function
    assert k(1, ONE + 1, 0, 8, fake) == -1 and 'threshold = 65537' in err()
    assert k(1, 6554, 0, 8, None) == -1 and 'null' in err()
    assert k(1, 6554, 0, 0, None) == 0


def test_the_binding_refuses_host_tensors_and_mismatched_operands():
    with pytest.raises(cabi.FewbitHipError, match='GPU'):
        cabi_x.dropout_apply(torch.zeros(8), 1, 0.5)
    with pytest.raises(cabi.FewbitHipError, match='between 0 and 1'):
        cabi_x.dropout_keep(1, 8, 1.5)


# ---- fewbit_amd.dropout on the host ----------------------------------------------------------------------------------------------------
def test_a_host_tensor_takes_torch_dropout_unchanged():
    x = torch.randn(7, 33)
    for inplace in (False, True):
        torch.manual_seed(5)
        got = fewbit.functional.dropout(x.clone(), 0.3, inplace=inplace)
        torch.manual_seed(5)
        assert torch.equal(got, F.dropout(x.clone(), 0.3, inplace=inplace))
    r = torch.randn(7, 33)
    torch.manual_seed(6)
    got = fewbit.functional.dropout_add(x, r, 0.3)
    torch.manual_seed(6)
    assert torch.equal(got, r + F.dropout(x, 0.3))
    xd = x.double().requires_grad_()
    torch.manual_seed(7)
    y = fewbit.dropout(xd, 0.5)
    y.sum().backward()
    assert torch.equal(xd.grad == 0, y == 0)
    assert fewbit.dropout is fewbit.functional.dropout and fewbit.dropout_add is fewbit.functional.dropout_add
    module = importlib.import_module('fewbit_amd.dropout')           # (the package attribute of that name is the function)
    assert module.dropout is fewbit.dropout and module.Dropout is fewbit.Dropout


@pytest.mark.parametrize('p', (-0.1, 1.1, float('nan')))
def test_p_is_validated_with_torchs_text(p):
    x, text = torch.ones(4), 'dropout probability has to be between 0 and 1, but got'
    for call in (lambda: fewbit.functional.dropout(x, p), lambda: fewbit.functional.dropout(x, p, training=False),
                 lambda: fewbit.functional.dropout_add(x, x, p)):
        with pytest.raises(ValueError, match=text):
            call()
    if p == p:                                                       # (nn.Dropout's constructor compares, and a NaN passes comparisons)
        with pytest.raises(ValueError, match=text):
            fewbit.Dropout(p)


def test_eval_mode_and_p_zero_draw_no_seed_and_return_the_values():
    x, r = torch.randn(5, 4, requires_grad=True), torch.randn(5, 4)
    torch.manual_seed(9)
    before = torch.get_rng_state()
    for y in (fewbit.functional.dropout(x, 0.5, training=False), fewbit.functional.dropout(x, 0.0), fewbit.Dropout(0.5).eval()(x)):
        assert y is x
    assert torch.equal(fewbit.functional.dropout_add(x, r, 0.5, training=False), r + x)
    assert torch.equal(fewbit.functional.dropout_add(x, r, 0.0), r + x)
    assert torch.equal(torch.get_rng_state(), before)
    assert not torch.equal(fewbit.functional.dropout(x, 0.5), x) and not torch.equal(torch.get_rng_state(), before)
    assert bool((fewbit.functional.dropout(x, 1.0) == 0).all())


def test_the_module_is_an_nn_dropout_and_map_module_swaps_the_right_ones():
    m = fewbit.Dropout(0.25, inplace=True)
    assert isinstance(m, torch.nn.Dropout) and repr(m) == repr(torch.nn.Dropout(0.25, inplace=True)) == 'Dropout(p=0.25, inplace=True)'
    assert m.generator is None and fewbit.Dropout().p == 0.5 and not fewbit.Dropout().inplace
    x = torch.ones(64)
    assert m.eval()(x) is x and bool((m.train()(x.clone()) == 0).any())
    assert 'Dropout' not in fewbit.modules.__all__
    model = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.Dropout(0.1), torch.nn.Dropout1d(0.2), torch.nn.AlphaDropout(0.2),
                                torch.nn.Sequential(torch.nn.GELU(), torch.nn.Dropout(0.3, inplace=True)), fewbit.Dropout(0.4))
    model = fewbit.map_module(model, lambda m, path: fewbit.Dropout(m.p, m.inplace) if type(m) is torch.nn.Dropout else m)
    swapped = [m for m in model.modules() if type(m) is fewbit.Dropout]
    assert [(m.p, m.inplace) for m in swapped] == [(0.1, False), (0.3, True), (0.4, False)]
    assert not any(type(m) is torch.nn.Dropout for m in model.modules())
    assert type(model[2]) is torch.nn.Dropout1d and type(model[3]) is torch.nn.AlphaDropout
