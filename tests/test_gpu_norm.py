"""The layer-norm entry points of the companion library on the GPU (include/fewbit_hipx.h, "the normalized rows of a seed";
fewbit_amd/csrc/fewbit_norm.hip), at every width at which the launch plan changes and on both sides of it, rows that do and do not fill a tile,
the three dtypes, the three code widths, pointers 0 and 1 element off 16-byte alignment, gamma / beta present and absent, the seed as an int
and as a device word.

* The state is bit for bit ``norm_state_host`` of the x^ the kernel hands out; nothing outside the buffers is written (guard bytes).
* x^ and rstd against float64 within ``K * 2^-24 * (|x^| + |mean| rstd + 1)`` (rstd: relative), K = max(2 K_ref, log2(width) + 4) with K_ref
  the smallest K that plain fp32 torch ops for the same formulas satisfy on the same inputs (torch sums in another order; a tree sum of
  `width` terms carries log2(width) roundings).  y within ``u |y| + that bound * |gamma| + 2^-24 |beta|``, which torch's own ``F.layer_norm``
  is asserted to keep as well.
* Backward from a given (host) state: dx against the float64 formula on ``norm_state_unpack_host`` within
  ``u |dx| + K' 2^-24 rstd (|g^| + mean|g^| + |x^q| mean|g^ x^q|)``, K' measured the same way; dgamma and dbeta within
  ``(rows + 3) 2^-24 sum_r |terms|``, the bound of a fixed-order fp32 sum of `rows` rounded products; two runs byte-equal; NULL outputs skipped.
* A workgroup that walks several tiles, at every lanes-per-row of the plan above 8 (``norm_harness.walk`` says where a walk begins and, backward,
  asserts it from the workspace query): backward a second and a third tile and three full sweeps by the bounds above; forward one row past one
  or two sweeps, the long call's rows byte for byte those of a call of its 37 distinct rows, which is held to float64, and the state that of the
  x^ handed out.
* A finite row whose centred squares overflow: rstd = 0, x^ = +-0, y = beta.
The measured K and K' are printed (EXPERIMENTS.md 8.18 and 8.25 record them)."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fewbit_amd import cabi_x
from norm_harness import DEV, EPS, FILL, SEED, UNIT, Guarded, allowance, backward_walks_on, forward_walks_on, options, seed_argument, state_rows, walks

pytestmark = pytest.mark.gpu
# 64 | 65, 128 | 129, 512 | 513, 1024 | 1025, 2048 | 2049, 4096 | 4097: one width on each side of every threshold of the plan (cabi_x.norm_plan)
WIDTHS = (1, 7, 8, 9, 63, 64, 65, 128, 129, 200, 512, 513, 768, 770, 1024, 1025, 2048, 2049, 4096, 4097, 8192)
ROWS = (1, 3, 37)
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
BITS = (2, 4, 8)
EPS32 = float(np.float32(EPS))
ids = lambda d: str(d).split('.')[-1] if isinstance(d, torch.dtype) else None


def inputs(rows, width, dtype, salt=0, kind='normal'):
    g = torch.Generator().manual_seed(1000 * width + rows + salt)
    x = 3 + 2 * torch.randn(rows, width, generator=g) if kind == 'normal' else 1000 + torch.randn(rows, width, generator=g)
    gamma, beta = 1 + 0.5 * torch.randn(width, generator=g), torch.randn(width, generator=g)
    return x.to(dtype), gamma.to(dtype), beta.to(dtype)


def reference64(x, gamma, beta):
    """float64 on the host from the stored values: mean, rstd, x^, y"""
    x = x.double().cpu()
    mean = x.mean(dim=1, keepdim=True)
    centred = x - mean
    rstd = 1.0 / torch.sqrt(centred.square().mean(dim=1, keepdim=True) + EPS32)
    xhat = centred * rstd
    y = xhat * (1.0 if gamma is None else gamma.double().cpu()) + (0.0 if beta is None else beta.double().cpu())
    return mean, rstd, xhat, y


def plain_fp32(x):
    """the same formulas as plain fp32 torch ops on the GPU: (x^, rstd)"""
    x = x.float()
    centred = x - x.mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(centred.square().mean(dim=1, keepdim=True) + EPS32)
    return (centred * rstd).double().cpu(), rstd.double().cpu()


def run_forward(x, gamma, beta, bits, seed, off, keep=True, want_xhat=True):
    """the call into guarded buffers -> (y, rstd, state, xhat) as Guarded (state / xhat: None when not asked for), after the guards were checked"""
    rows, width = x.shape
    gx = Guarded(x.numel(), x.dtype, off, x)
    gg = None if gamma is None else Guarded(width, x.dtype, off, gamma)
    gb = None if beta is None else Guarded(width, x.dtype, off, beta)
    y, rstd = Guarded(x.numel(), x.dtype, off), Guarded(rows, torch.float32, off)
    state = Guarded(cabi_x.norm_state_bytes(rows, width, bits), torch.uint8, 8 * off) if keep else None
    xhat = Guarded(x.numel(), torch.float32, off) if want_xhat else None
    cabi_x.layer_norm_forward(gx.t.view(rows, width), None if gg is None else gg.t, None if gb is None else gb.t, EPS, bits, seed, keep=keep,
                              y=y.t.view(rows, width), rstd=rstd.t, state=None if state is None else state.t, xhat=None if xhat is None else xhat.t.view(rows, width))
    torch.cuda.synchronize()
    for name, buffer in (('y', y), ('rstd', rstd), ('state', state), ('xhat', xhat)):
        assert buffer is None or buffer.intact(), f'{name}: guard bytes were written'
    for name, buffer in (('x', gx), ('gamma', gg), ('beta', gb)):
        assert buffer is None or buffer.unchanged(), f'{name} was written'
    return y, rstd, state, xhat


def check_forward_values(x, gamma, beta, y, rstd, xhat, label):
    """x^, rstd and y against float64 by the bounds of the module docstring -> (K of x^, K of rstd, their reference values)"""
    rows, width = x.shape
    mean, rstd64, xhat64, y64 = reference64(x, gamma, beta)
    unit = 2.0**-24 * (xhat64.abs() + mean.abs() * rstd64 + 1.0)
    ref_xhat, ref_rstd = plain_fp32(x.to(DEV))
    k_ref = float(((ref_xhat - xhat64).abs() / unit).max())
    k_ref_rstd = float(((ref_rstd - rstd64).abs() / (2.0**-24 * rstd64)).max())
    k = float(((xhat.double().cpu() - xhat64).abs() / unit).max())
    k_rstd = float(((rstd.double().cpu().view(-1, 1) - rstd64).abs() / (2.0**-24 * rstd64)).max())
    allowed = allowance(max(k_ref, k_ref_rstd), width)
    assert k <= allowed and k_rstd <= allowed, f'{label}: K = {k:.2f}, K(rstd) = {k_rstd:.2f}; allowed {allowed:.2f} (plain fp32 ops: {k_ref:.2f}, {k_ref_rstd:.2f})'
    bound = UNIT[x.dtype] * y64.abs() + allowed * unit * (1.0 if gamma is None else gamma.double().cpu().abs()) + (0.0 if beta is None else 2.0**-24 * beta.double().cpu().abs())
    theirs = F.layer_norm(x.to(DEV), (width, ), None if gamma is None else gamma.to(DEV), None if beta is None else beta.to(DEV), EPS)
    assert bool(((theirs.double().cpu() - y64).abs() <= bound).all()), f'{label}: torch\'s layer_norm leaves the bound'
    worst = float(((y.double().cpu() - y64).abs() / bound).max())
    assert worst <= 1.0, f'{label}: y is {worst:.3f} bounds off'
    return k, k_rstd, k_ref, k_ref_rstd


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('dtype', DTYPES, ids=ids)
def test_forward_state_values_and_guards(dtype, bits):
    worst = [0.0, 0.0, 0.0, 0.0]
    for i, (width, rows) in enumerate(itertools.product(WIDTHS, ROWS)):
        off, affine, device_word = options(i)
        x, gamma, beta = inputs(rows, width, dtype)
        gamma, beta = (gamma, beta) if affine else (None, None)
        label = f'{rows} x {width} off {off} affine {affine} device word {device_word}'
        y, rstd, state, xhat = run_forward(x, gamma, beta, bits, seed_argument(device_word), off)
        # the state, bit for bit, from the x^ the kernel quantized
        want = cabi_x.norm_state_host(xhat.t.view(rows, width).cpu(), SEED, bits)
        got = state.t.cpu()
        assert torch.equal(got, want), f'{label}: state differs at bytes {torch.nonzero(got != want).flatten()[:8].tolist()}'
        ks = check_forward_values(x, gamma, beta, y.t.view(rows, width), rstd.t, xhat.t.view(rows, width), label)
        worst = [max(a, b) for a, b in zip(worst, ks)]
        # the plain forward: the same y and rstd bytes, nothing else
        y0, rstd0, _, _ = run_forward(x, gamma, beta, bits, SEED, off, keep=False, want_xhat=False)
        assert torch.equal(y0.raw, y.raw) and torch.equal(rstd0.raw, rstd.raw), label
        # the same arguments, the same bytes
        again = run_forward(x, gamma, beta, bits, SEED, off)
        assert all(torch.equal(a.raw, b.raw) for a, b in zip(again, (y, rstd, state, xhat))), label
    print(f'{dtype} bits {bits}: K(x^) = {worst[0]:.2f}, K(rstd) = {worst[1]:.2f}; plain fp32 torch ops: {worst[2]:.2f}, {worst[3]:.2f}')


def backward_problem(rows, width, dtype, bits, affine, salt=0):
    g = torch.Generator().manual_seed(7000 * width + rows + salt)
    xhat = torch.randn(rows, width, generator=g)
    state = cabi_x.norm_state_host(xhat, SEED + salt, bits)
    xq = cabi_x.norm_state_unpack_host(state, rows, width, bits)
    rstd = 0.25 + torch.rand(rows, generator=g)
    gy = torch.randn(rows, width, generator=g).to(dtype)
    gamma = (1 + 0.5 * torch.randn(width, generator=g)).to(dtype) if affine else None
    return state, xq, rstd, gy, gamma


def run_backward(state, rstd, gy, gamma, bits, off, want=(True, True, True), workspace=None):
    rows, width = gy.shape
    g_gy, g_state, g_rstd = Guarded(gy.numel(), gy.dtype, off, gy), Guarded(state.numel(), torch.uint8, 8 * off, state), Guarded(rows, torch.float32, off, rstd)
    g_gamma = None if gamma is None else Guarded(width, gy.dtype, off, gamma)
    dx = Guarded(gy.numel(), gy.dtype, off) if want[0] else None
    dgamma = Guarded(width, torch.float32, off) if want[1] else None
    dbeta = Guarded(width, torch.float32, off) if want[2] else None
    cabi_x.layer_norm_backward(g_gy.t.view(rows, width), g_state.t, g_rstd.t, None if g_gamma is None else g_gamma.t, bits, want,
                               dx=None if dx is None else dx.t.view(rows, width), dgamma=None if dgamma is None else dgamma.t,
                               dbeta=None if dbeta is None else dbeta.t, workspace=workspace)
    torch.cuda.synchronize()
    for name, buffer in (('dx', dx), ('dgamma', dgamma), ('dbeta', dbeta)):
        assert buffer is None or buffer.intact(), f'{name}: guard bytes were written'
    for name, buffer in (('gy', g_gy), ('state', g_state), ('rstd', g_rstd), ('gamma', g_gamma)):
        assert buffer is None or buffer.unchanged(), f'{name} was written'
    return dx, dgamma, dbeta


def check_backward_values(xq, rstd, gy, gamma, dx, dgamma, dbeta, label):
    rows, width = gy.shape
    gy64, xq64, rstd64 = gy.double(), xq.double(), rstd.double().view(-1, 1)
    gh = gy64 * (1.0 if gamma is None else gamma.double())
    dx64 = rstd64 * (gh - gh.mean(dim=1, keepdim=True) - xq64 * (gh * xq64).mean(dim=1, keepdim=True))
    unit = 2.0**-24 * rstd64 * (gh.abs() + gh.abs().mean(dim=1, keepdim=True) + xq64.abs() * (gh * xq64).abs().mean(dim=1, keepdim=True))
    # plain fp32 torch ops on the GPU for the same formula
    g32 = gy.to(DEV).float() * (1.0 if gamma is None else gamma.to(DEV).float())
    q32, r32 = xq.to(DEV), rstd.to(DEV).view(-1, 1)
    ref = (r32 * (g32 - g32.mean(dim=1, keepdim=True) - q32 * (g32 * q32).mean(dim=1, keepdim=True))).double().cpu()
    k_ref = float(((ref - dx64).abs() / unit).max())
    allowed = allowance(k_ref, width)
    err = (dx.double().cpu() - dx64).abs()
    k = float(((err - UNIT[gy.dtype] * dx64.abs()).clamp_min(0) / unit).max())
    assert k <= allowed, f"{label}: K' = {k:.2f}, allowed {allowed:.2f} (plain fp32 ops: {k_ref:.2f})"
    terms = gy64 * xq64
    assert bool(((dgamma.double().cpu() - terms.sum(dim=0)).abs() <= (rows + 3) * 2.0**-24 * terms.abs().sum(dim=0)).all()), f'{label}: dgamma'
    assert bool(((dbeta.double().cpu() - gy64.sum(dim=0)).abs() <= (rows + 3) * 2.0**-24 * gy64.abs().sum(dim=0)).all()), f'{label}: dbeta'
    return k, k_ref


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('dtype', DTYPES, ids=ids)
def test_backward_from_a_given_state(dtype, bits):
    worst = [0.0, 0.0]
    for i, (width, rows) in enumerate(itertools.product(WIDTHS, ROWS)):
        off, affine, _ = options(i)
        state, xq, rstd, gy, gamma = backward_problem(rows, width, dtype, bits, affine)
        label = f'{rows} x {width} off {off} affine {affine}'
        dx, dgamma, dbeta = run_backward(state, rstd, gy, gamma, bits, off)
        ks = check_backward_values(xq, rstd, gy, gamma, dx.t.view(rows, width), dgamma.t, dbeta.t, label)
        worst = [max(a, b) for a, b in zip(worst, ks)]
        again = run_backward(state, rstd, gy, gamma, bits, off)
        assert all(torch.equal(a.raw, b.raw) for a, b in zip(again, (dx, dgamma, dbeta))), f'{label}: two runs differ'
        # NULL outputs are skipped: the others keep their bytes, and with neither sum the workspace is not touched
        scratch = torch.full((cabi_x.norm_workspace_bytes(rows, width), ), FILL, dtype=torch.uint8, device=DEV)
        only_dx, none_g, none_b = run_backward(state, rstd, gy, gamma, bits, off, (True, False, False), scratch)
        assert none_g is None and none_b is None and torch.equal(only_dx.raw, dx.raw) and bool((scratch == FILL).all()), label
        none_dx, only_g, only_b = run_backward(state, rstd, gy, gamma, bits, off, (False, True, True))
        assert none_dx is None and torch.equal(only_g.raw, dgamma.raw) and torch.equal(only_b.raw, dbeta.raw), label
        if i % 8 == 0:
            _, only_g, none_b = run_backward(state, rstd, gy, gamma, bits, off, (False, True, False))
            assert none_b is None and torch.equal(only_g.raw, dgamma.raw), label
    print(f"{dtype} bits {bits}: K'(dx) = {worst[0]:.2f}; plain fp32 torch ops: {worst[1]:.2f}")


@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16), ids=ids)
def test_width_8_one_row_past_a_full_sweep_of_the_grid(dtype):
    """32 rows of width 8 share a forward workgroup, 128 a backward one: forward sweeps 16384 * 32 rows at once, backward 512 * 128; one row more
    than the longer sweep starts the next one of both"""
    rows, width, bits = 16384 * 32 + 1, 8, 4
    x, gamma, beta = inputs(rows, width, dtype)
    y, rstd, state, xhat = run_forward(x, gamma, beta, bits, SEED, 0)
    assert torch.equal(state.t.cpu(), cabi_x.norm_state_host(xhat.t.view(rows, width).cpu(), SEED, bits))
    check_forward_values(x, gamma, beta, y.t.view(rows, width), rstd.t, xhat.t.view(rows, width), 'the long sweep')
    host_state, xq, rstd_given, gy, gamma = backward_problem(rows, width, dtype, bits, True)
    dx, dgamma, dbeta = run_backward(host_state, rstd_given, gy, gamma, bits, 1)
    check_backward_values(xq, rstd_given, gy, gamma, dx.t.view(rows, width), dgamma.t, dbeta.t, 'the long sweep')


@pytest.mark.parametrize('case', walks('backward'), ids=str)
def test_backward_a_workgroup_walks_on_at_every_lanes_per_row(case):
    """16 to 1024 lanes per row, 512 workgroups (asserted from the workspace query): one row past one and past two sweeps -- workgroup 0 alone walks on,
    with one live row in a tile of dead lanes; its third tile writes the slots of the first again -- and three full sweeps.  The column accumulators
    are carried across the tiles into the direct store (1 row per tile), the LDS column loop (2 or 4 rows per tile: more than one trip) or the plain
    one, and 512 partials per column enter the column sums"""
    backward_walks_on(case, backward_problem, run_backward, check_backward_values)


@pytest.mark.parametrize('case', walks('forward'), ids=str)
def test_forward_a_workgroup_walks_on_at_every_lanes_per_row(case):
    """16 to 256 lanes per row and 1, 2 or 4 blocks per lane, one row past one or two sweeps of the 16384 workgroups (norm_harness.forward_walks_on)"""
    forward_walks_on(case, inputs, run_forward, check_forward_values)


@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16), ids=ids)
def test_a_finite_row_whose_centred_squares_overflow_gives_rstd_0_and_y_beta(dtype):
    """A row of alternating +-2^66 at an even width: its sum is exactly 0, so the mean is 0 and only the squares of the centred row overflow.
    var = inf, rstd = 0, x^ = +-0 (nothing is NaN, no group is poisoned), y = beta; backward from that state: dx of the row is 0, dgamma is
    finite and the bytes of the same call without the row's gy.  Every other row has the bytes of a run where the row holds ordinary values"""
    rows, width, bits, at = 5, 200, 4, 2
    clean, gamma, beta = inputs(rows, width, dtype, 5)
    x = clean.clone()
    x[at] = (2.0**66 * (1 - 2 * (torch.arange(width) % 2))).to(dtype)
    gy = torch.randn(rows, width, generator=torch.Generator().manual_seed(11)).to(dtype)
    others = [r for r in range(rows) if r != at]
    y, rstd, state, xhat = run_forward(x, gamma, beta, bits, SEED, 0)
    y0, rstd0, state0, xhat0 = run_forward(clean, gamma, beta, bits, SEED, 0)
    assert float(rstd.t[at]) == 0.0 and not bool(xhat.t.view(rows, width)[at].any()) and torch.equal(y.t.view(rows, width)[at].cpu(), beta)
    xq = cabi_x.norm_state_unpack_host(state.t.cpu(), rows, width, bits)
    assert not bool(torch.isnan(xq).any()) and not bool(xq[at].any())
    assert all(torch.equal(a[others], b[others]) for a, b in zip(state_rows(state.t, rows, width), state_rows(state0.t, rows, width)))
    for a, b in ((y, y0), (xhat, xhat0), (rstd, rstd0)):
        assert torch.equal(a.t.view(rows, -1)[others].view(torch.uint8), b.t.view(rows, -1)[others].view(torch.uint8))
    dx, dgamma, dbeta = run_backward(state.t, rstd.t, gy, gamma, bits, 0)
    dx0 = run_backward(state0.t, rstd0.t, gy, gamma, bits, 0)[0]
    assert not bool(dx.t.view(rows, width)[at].any()) and torch.equal(dx.t.view(rows, width)[others], dx0.t.view(rows, width)[others])
    without = gy.clone()
    without[at] = 0
    assert bool(torch.isfinite(dgamma.t).all()) and torch.equal(run_backward(state.t, rstd.t, without, gamma, bits, 0)[1].raw, dgamma.raw)


@pytest.mark.parametrize('bits', BITS)
def test_value_edges(bits):
    rows, width = 6, 200
    # a constant row: x^ = 0, every code 0, rstd = 1 / sqrt(eps)
    x = torch.full((rows, width), 3.25)
    y, rstd, state, xhat = run_forward(x, None, None, bits, SEED, 0)
    assert not bool(xhat.t.any()) and not bool(state.t.any()) and not bool(y.t.any())
    assert rstd.t.cpu().numpy().tolist() == [float(np.float32(1) / np.sqrt(np.float32(EPS)))] * rows
    # rows of 1000 + N(0, 1) in fp32 stay inside the bound of x^ (the variance is the two-pass one)
    x, gamma, beta = inputs(rows, width, torch.float32, kind='offset')
    y, rstd, state, xhat = run_forward(x, gamma, beta, bits, SEED, 1)
    k = check_forward_values(x, gamma, beta, y.t.view(rows, width), rstd.t, xhat.t.view(rows, width), '1000 + N(0, 1)')
    print(f'bits {bits}: rows of 1000 + N(0, 1): K(x^) = {k[0]:.2f}, K(rstd) = {k[1]:.2f}; plain fp32 torch ops: {k[2]:.2f}, {k[3]:.2f}')
    # denormal rows give no NaN
    tiny = (torch.randn(rows, width) * 1e-40).float()
    y, rstd, state, xhat = run_forward(tiny, gamma, beta, bits, SEED, 0)
    assert not bool(torch.isnan(y.t).any()) and not bool(torch.isnan(xhat.t).any()) and not bool(torch.isnan(rstd.t).any())
    assert not bool(torch.isnan(cabi_x.norm_state_unpack_host(state.t.cpu(), rows, width, bits)).any())


@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16), ids=ids)
@pytest.mark.parametrize('poison', ('nan', 'inf'))
def test_a_non_finite_row_is_nan_and_touches_no_other(poison, dtype):
    rows, width, bits = 5, 200, 4
    clean, gamma, beta = inputs(rows, width, dtype, 3)
    x = clean.clone()
    x[2, 77] = float(poison)
    gy = torch.randn(rows, width).to(dtype)
    results = []
    for source in (clean, x):
        y, rstd, state, xhat = run_forward(source, gamma, beta, bits, SEED, 0)
        dx, dgamma, dbeta = run_backward(state.t, rstd.t, gy, gamma, bits, 0)
        results.append((y.t.view(rows, width).clone(), dx.t.view(rows, width).clone(), dgamma.t.clone(), dbeta.t.clone(), xhat.t.view(rows, width).clone()))
    (y0, dx0, dgamma0, dbeta0, _), (y1, dx1, dgamma1, dbeta1, xhat1) = results
    others = [0, 1, 3, 4]
    assert bool(torch.isnan(y1[2]).all()) and bool(torch.isnan(dx1[2]).all()) and bool(torch.isnan(xhat1[2]).all())
    assert bool(torch.isnan(dgamma1).all())                             # the row touches every column
    assert torch.equal(dbeta1, dbeta0) and not bool(torch.isnan(dgamma0).any())
    assert torch.equal(y1[others], y0[others]) and torch.equal(dx1[others], dx0[others])
