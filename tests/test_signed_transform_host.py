"""The sampled transforms behind a random sign per row (S = sqrt(N / p) R T D) without a GPU: the signs of a seed against Philox, their
balance, the identity that keeps the estimator unbiased, the variance the signs are there for, the switch of the layer, and the layer's
PyTorch formulation with the switch on -- all in float64 on the host."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.fft
import torch
import torch.nn.functional as F

import sketch_reference as ref
from fewbit_amd import cabi, cabi_x, linear
from helpers import ROOT

SEEDS = (0, 20261019, 0x9E3779B97F4A7C15)
SIGNED_SYMBOLS = ('fewbit_hipx_sampled_signs', 'fewbit_hipx_sampled_dct_signed', 'fewbit_hipx_sampled_dft_signed')


def signs_of_philox(seed: int, first: int, count: int) -> np.ndarray:
    """the definition of include/fewbit_hipx.h ("the signs of a seed") on the Philox of tests/sketch_reference.py"""
    r = np.uint64(first) + np.arange(count, dtype=np.uint64)
    q = r >> np.uint64(7)
    w = np.stack(ref.philox4x32(q & ref.M32, q >> np.uint64(32), 0, 6, *ref._key(seed)))
    word = w[((r >> np.uint64(5)) & np.uint64(3)).astype(np.int64), np.arange(count)]
    return ((word >> (r & np.uint64(31))) & np.uint64(1)).astype(bool)


def transform(kind: str, m: np.ndarray) -> np.ndarray:
    return scipy.fft.dct(m, axis=0, norm='ortho') if kind == 'dct' else np.fft.fft(m, axis=0, norm='ortho')


def flipped(m: np.ndarray, flip: np.ndarray) -> np.ndarray:
    return np.where(flip[:, None], -m, m)


@pytest.mark.parametrize('seed', SEEDS)
def test_the_signs_are_the_philox_bits_of_the_definition(seed):
    """bit by bit, over ranges that cross a 32-row word, a 128-row Philox block and the block 2^32 (row 2^39: counter word 1 becomes 1)"""
    for first, count in ((0, 700), (25, 20), (100, 60), (127, 2), ((1 << 39) - 300, 600), ((1 << 39) + (1 << 7) - 1, 2), ((1 << 63) + 5, 200)):
        got = cabi_x.sampled_signs(seed, count, first).numpy()
        want = signs_of_philox(seed, first, count)
        assert got.dtype == np.bool_ and np.array_equal(got, want), (seed, first)
    # counter word 1 matters: the rows 2^39 apart do not repeat
    assert not np.array_equal(cabi_x.sampled_signs(seed, 512).numpy(), cabi_x.sampled_signs(seed, 512, 1 << 39).numpy())


@pytest.mark.parametrize('seed', SEEDS)
def test_slices_of_the_signs_agree_with_the_whole(seed):
    whole = cabi_x.sampled_signs(seed, 1000)
    for first, count in ((0, 1), (0, 33), (31, 2), (96, 64), (127, 129), (999, 1), (500, 0)):
        assert torch.equal(cabi_x.sampled_signs(seed, count, first), whole[first:first + count]), (first, count)
    high = cabi_x.sampled_signs(seed, 400, (1 << 39) - 200)
    assert torch.equal(cabi_x.sampled_signs(seed, 100, (1 << 39) - 50), high[150:250])
    assert cabi_x.sampled_signs(seed, 0).numel() == 0
    with pytest.raises(cabi.FewbitHipError):
        cabi_x.sampled_signs(seed, -1)


@pytest.mark.parametrize('seed', SEEDS)
def test_the_signs_are_balanced(seed):
    """the share of flips over 2^20 rows is within 4 standard deviations (4 x 0.5 / 2^10) of 1/2"""
    n = 1 << 20
    share = float(cabi_x.sampled_signs(seed, n).double().mean())
    z = (share - 0.5) / (0.5 / np.sqrt(n))
    print(f'seed {seed:#x}: share of flipped rows {share:.6f} ({z:+.2f} standard deviations)')
    assert abs(z) <= 4.0


@pytest.mark.parametrize('kind', ('dct', 'dft'))
@pytest.mark.parametrize('n', (256, 768))
def test_the_signed_transform_keeps_the_product(kind, n):
    """sum_k (T D G)_k^H (T D X)_k = G^T X to 1e-12 relative: E[S^T S] = D T^H T D = I for every D"""
    rng = np.random.default_rng(n)
    x, g = rng.standard_normal((n, 8)), rng.standard_normal((n, 5))
    for seed in SEEDS:
        flip = cabi_x.sampled_signs(seed, n).numpy()
        tx, tg = transform(kind, flipped(x, flip)), transform(kind, flipped(g, flip))
        got, want = (tg.conj().T @ tx), g.T @ x
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f'{kind} N = {n} seed {seed:#x}: relative deviation {err:.2e}')
        assert err <= 1e-12


def variance_factor(kind: str, x: np.ndarray, g: np.ndarray) -> float:
    """N sum_k |(T G)_k|^2 |(T X)_k|^2 / (|G|^2 |X|^2): the leading term of the estimator's variance as a multiple of the dense sketches'"""
    tx, tg = transform(kind, x), transform(kind, g)
    return float(x.shape[0] * ((np.abs(tg)**2).sum(1) * (np.abs(tx)**2).sum(1)).sum() / ((g**2).sum() * (x**2).sum()))


@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_the_signs_bound_the_variance_of_an_input_with_a_mean(kind):
    """columns of 1 + 0.01 noise at N = 256 (8 features, 5 gradient columns): without signs the factor is at least N / 2 (it is N: all the
    energy in transform row 0); with D = sampled_signs(seed, 256) it is at most 6 for each of the seeds 0 .. 19 (twice the limit 3 of a
    rank-one input under a real transform)"""
    n = 256
    rng = np.random.default_rng(7)
    x, g = 1 + 0.01 * rng.standard_normal((n, 8)), 1 + 0.01 * rng.standard_normal((n, 5))
    plain = variance_factor(kind, x, g)
    print(f'{kind}: factor without signs {plain:.1f}')
    assert plain >= n / 2
    worst = 0.0
    for seed in range(20):
        flip = cabi_x.sampled_signs(seed, n).numpy()
        factor = variance_factor(kind, flipped(x, flip), flipped(g, flip))
        print(f'{kind}: seed {seed}: factor with signs {factor:.3f}')
        worst = max(worst, factor)
        assert factor <= 6.0, (seed, factor)
    print(f'{kind}: largest factor with signs over 20 seeds {worst:.3f}')


def test_the_switch_is_off_by_default_and_returns_its_previous_value():
    assert 'FEWBIT_SIGN_FLIPS' not in os.environ or os.environ['FEWBIT_SIGN_FLIPS'] in ('0', '')
    assert linear.use_sign_flips() is False
    x = torch.zeros(300, 8)
    off = linear.sampled_transform_path('dct', x)
    assert linear.use_sign_flips(True) is False
    try:
        assert linear.use_sign_flips() is True
        on = linear.sampled_transform_path('dct', x)
        assert 'signs' in on and on != off
        assert linear.use_sign_flips(False) is True
    finally:
        linear.use_sign_flips(False)
    assert linear.use_sign_flips() is False and linear.sampled_transform_path('dct', x) == off


def test_the_environment_variable_sets_the_switch_in_a_child_process():
    for value, want in (('1', True), ('0', False), (None, False)):
        env = {k: v for k, v in os.environ.items() if k != 'FEWBIT_SIGN_FLIPS'}
        if value is not None:
            env['FEWBIT_SIGN_FLIPS'] = value
        code = 'import sys; sys.path.insert(0, %r)\nfrom fewbit_amd import linear\nprint(linear.use_sign_flips())' % str(ROOT)
        r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and r.stdout.strip() == str(want), (value, r.stdout, r.stderr[-2000:])


def test_a_library_without_the_symbols_is_refused_by_name():
    code = ('import os, sys; sys.path.insert(0, %r)\n'
            'os.environ["FEWBIT_HIPX_LIB"] = %r\n'
            'from fewbit_amd import cabi_x, cabi\n'
            'try:\n    cabi_x.lib()\nexcept cabi.FewbitHipError as e:\n    assert all(name in str(e) for name in %r), e\n'
            'else:\n    raise SystemExit("loaded")' % (str(ROOT), str(cabi.LIB_PATH), SIGNED_SYMBOLS))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_the_library_exports_the_signed_entry_points_inside_revision_2():
    out = subprocess.run(['nm', '-D', '--defined-only', str(cabi_x.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SIGNED_SYMBOLS) <= exported and set(SIGNED_SYMBOLS) <= set(cabi_x.SYMBOLS)
    assert cabi_x.lib().fewbit_hipx_revision() == cabi_x.REVISION == 2


def test_signed_calls_are_refused_by_name_before_anything_is_launched():
    """the refusals of the _zext_seeded entry points, the same codes, with the new names in the message (no device is touched)"""
    L = cabi_x.lib()
    err = L.fewbit_hipx_last_error
    dct, dft = L.fewbit_hipx_sampled_dct_signed, L.fewbit_hipx_sampled_dft_signed
    need = cabi_x.sampled_dft_workspace_bytes(3072, 8, 4, torch.float32)
    assert dct(0, 16, 3000, 10, 8, 8, 1, None, 4, 1.0, 16, 16, 1 << 30, None) == -2 and b'rows = 3000' in err() and b'sampled_dct_signed' in err()
    assert dft(0, 16, 300, 10, 8, 8, 1, None, 4, 1.0, 0, 16, 16, 1 << 30, None) == -2 and b'rows = 300' in err() and b'sampled_dft_signed' in err()
    for valid in (0, 3073, 1 << 40):
        assert dct(1, 16, 3072, valid, 8, 8, 1, None, 4, 1.0, 16, 16, 1 << 30, None) == -1 and b'valid_rows' in err() and b'sampled_dct_signed' in err()
        assert dft(0, 16, 3072, valid, 8, 8, 1, None, 4, 1.0, 0, 16, 16, 1 << 30, None) == -1 and b'valid_rows' in err() and b'sampled_dft_signed' in err()
    assert dct(9, 16, 3072, 3000, 8, 8, 1, None, 4, 1.0, 16, 16, 1 << 30, None) == -1 and b'dtype' in err()
    assert dft(2, 16, 3072, 3000, 8, 8, 1, None, 4, 1.0, 1, 16, 16, 1 << 30, None) == -1 and b'out_dtype' in err() and b'sampled_dft_signed' in err()
    assert dct(0, 16, 3072, 3000, 8, 8, 1, None, 4, 1.0, 16, 16, need - 1, None) == -1 and b'workspace' in err()
    assert dft(0, 16, 3072, 3000, 8, 8, 1, None, 4, 1.0, 0, 16, None, 0, None) == -1 and b'workspace' in err()
    assert dft(0, 16, 3072, 3000, 8, 8, 1, None, 4, 1.0, 0, 16, 24, need + 64, None) == -1 and b'aligned' in err()
    assert dct(0, None, 3072, 3000, 8, 8, 1, None, 4, 1.0, 16, 16, need, None) == -1 and b'null' in err()
    assert dct(0, 16, 3072, 3000, 8, 7, 1, None, 4, 1.0, 16, 16, need, None) == -1 and b'leading dimension' in err()
    assert dft(0, 16, 3072, 3000, 8, 8, 1, 12, 4, 1.0, 0, 16, 16, need, None) == -1 and b'8-byte aligned' in err()
    assert dct(0, 16, 3072, 3000, 8, 1 << 20, 1, None, 4, 1.0, 16, 16, need, None) == -2 and b'4 GiB' in err()
    assert dct(0, None, 3000, 0, 8, 8, 1, None, 0, 1.0, None, None, 0, None) == 0             # nothing to do: no samples
    assert L.fewbit_hipx_sampled_signs(1, 0, 4, None) == -1 and b'sampled_signs' in err()


# ---- the layer's PyTorch formulation with the switch on (host tensors, float64) -------------------------------------------------------
def model_grad_weight(kind: str, x: np.ndarray, g: np.ndarray, p: int, state: torch.Tensor, signed: bool) -> np.ndarray:
    """(S G)^T (S X), S = sqrt(N / p) R T D, in float64 with scipy / numpy transforms: D and then R replayed from the generator state the
    layer started from (D is drawn before the rows)"""
    n = x.shape[0]
    gen = torch.Generator()
    gen.set_state(state)
    if signed:
        flip = torch.randint(0, 2, (n, ), generator=gen, dtype=torch.int8).bool().numpy()
        x, g = flipped(x, flip), flipped(g, flip)
    idx = torch.randint(0, n, (p, ), generator=gen).numpy()
    tx, tg = transform(kind, x)[idx], transform(kind, g)[idx]
    return (n / p) * (tg.conj().T @ tx).real


@pytest.fixture
def sign_flips():
    prev = linear.use_sign_flips(True)
    yield
    linear.use_sign_flips(prev)


@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_the_host_layer_with_signs_is_exact_where_it_must_be_and_follows_the_model(kind, sign_flips):
    torch.manual_seed(3)
    n, f_in, f_out, p = 96, 6, 5, 40
    x = (1 + 0.1 * torch.randn(n, f_in, dtype=torch.float64)).requires_grad_()
    w = torch.randn(f_out, f_in, dtype=torch.float64, requires_grad=True)
    b = torch.randn(f_out, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(n, f_out, dtype=torch.float64)
    gen = torch.Generator().manual_seed(11)
    state = gen.get_state()
    y = linear.linear_grp(x, w, b, proj_dim=p, matmul=kind, generator=gen)
    assert torch.equal(y, F.linear(x, w, b))
    y.backward(gy)
    assert torch.equal(x.grad, gy @ w.detach()) and torch.equal(b.grad, gy.sum(0))
    want = model_grad_weight(kind, x.detach().numpy(), gy.numpy(), p, state, True)
    err = np.abs(w.grad.numpy() - want).max() / np.abs(want).max()
    print(f'{kind}: grad_weight against the float64 model: relative deviation {err:.2e}')
    assert err <= 1e-11
    unsigned = model_grad_weight(kind, x.detach().numpy(), gy.numpy(), p, state, False)
    assert np.abs(want - unsigned).max() > 1e-3 * np.abs(want).max()            # (the signs are not a no-op)


@pytest.mark.parametrize('kind', ('dct', 'dft'))
@pytest.mark.parametrize('forward_on', (True, False))
def test_backward_follows_what_the_forward_did_not_the_switch(kind, forward_on):
    torch.manual_seed(4)
    n, f_in, f_out, p = 64, 4, 3, 32
    x = torch.randn(n, f_in, dtype=torch.float64)
    w = torch.randn(f_out, f_in, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(n, f_out, dtype=torch.float64)
    gen = torch.Generator().manual_seed(12)
    state = gen.get_state()
    prev = linear.use_sign_flips(forward_on)
    try:
        y = linear.linear_grp(x, w, None, proj_dim=p, matmul=kind, generator=gen)
        linear.use_sign_flips(not forward_on)
        y.backward(gy)
    finally:
        linear.use_sign_flips(prev)
    want = model_grad_weight(kind, x.numpy(), gy.numpy(), p, state, forward_on)
    assert np.abs(w.grad.numpy() - want).max() <= 1e-11 * np.abs(want).max()


def test_the_dense_sketches_and_the_switch_off_are_untouched(sign_flips):
    """'gaussian' / 'rademacher' draw what they drew: the switch concerns the sampled transforms alone"""
    x = torch.randn(64, 4, dtype=torch.float64)
    w = torch.randn(3, 4, dtype=torch.float64)
    grads = []
    for on in (True, False):
        linear.use_sign_flips(on)
        for kind in ('gaussian', 'rademacher'):
            wl = w.clone().requires_grad_()
            linear.linear_grp(x, wl, None, proj_dim=16, matmul=kind, generator=torch.Generator().manual_seed(5)).sum().backward()
            grads.append(wl.grad)
    assert torch.equal(grads[0], grads[2]) and torch.equal(grads[1], grads[3])
