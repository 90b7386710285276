"""The RMS-norm entry points of the companion library on the GPU (include/fewbit_hipx.h, "The un-centred rows"; fewbit_amd/csrc/fewbit_norm.hip), by
the method of tests/test_gpu_norm.py: every width at which the launch plan changes and both sides of it, rows that do and do not fill a tile,
the three dtypes, the three code widths, pointers 0 and 1 element off 16-byte alignment, gamma present and absent, the seed as an int and as
a device word.

* The state is bit for bit ``norm_state_host`` of the x^ the kernel hands out; nothing outside the buffers is written (guard bytes).
* x^ and rstd against float64 from the stored values within ``K * 2^-24 * |x^|`` plus the smallest denormal (rstd: ``K * 2^-24`` relative),
  K = max(2 K_ref, log2(width) + 4) with K_ref the smallest K that plain fp32 torch ops for the same formulas satisfy on the same inputs (torch sums
  in another order; a tree sum of `width` terms carries log2(width) roundings).  y within ``u |y| + K 2^-24 |x^| |gamma|``; torch's own
  ``F.rms_norm`` is asserted to keep that bound in fp32 only, for 16-bit inputs its distance is printed (it may round x^ before the weight).
  ``u |y|`` is the error of the one rounding to the dtype; below the dtype's smallest normal number that error is half the spacing of its
  denormals instead (2^-25 in fp16), whatever |y| -- the correctly rounded float64 x^ of the 37 x 512 fp16 case is 1.019 of ``u |y|`` away at
  x = 1.0e-4, x^ = 2.9e-5 -- so the term is ``max(u |y|, half a denormal)``; likewise for dx.
* Backward from a given (host) state: dx against the float64 formula on ``norm_state_unpack_host`` within
  ``u |dx| + K' 2^-24 rstd (|g^| + |x^q| mean|g^ x^q|)``, K' measured the same way; dgamma within ``(rows + 3) 2^-24 sum_r |gy x^q|``, the bound
  of a fixed-order fp32 sum of `rows` rounded products; two runs byte-equal; NULL outputs skipped, and without dgamma the workspace untouched.
* A workgroup that walks several tiles with ONE row sum per tile through LDS (rows of 520 elements, 128 lanes per row): the slots of the row
  sum alternate between tiles, which the sweeps of 2 and of 3 tiles per workgroup would show if they did not.  The same at every other
  lanes-per-row of the plan above 8 -- the row sum of 4, 8 and 16 waves, 2 and 4 blocks per lane forward -- by the method of tests/test_gpu_norm.py
  (``norm_harness.walk``, ``backward_walks_on``, ``forward_walks_on``).
* A finite row whose sum of squares overflows: rstd = 0, x^ = y = +-0, no group poisoned.
The measured K and K' are printed (EXPERIMENTS.md 8.19 and 8.25 record them)."""
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
TINY = 2.0**-149                                                      # the smallest fp32 denormal
# half the spacing of the dtype's denormals: what ONE correct rounding to the dtype may err by where u |value| is smaller than that (a y or dx below
# the smallest normal number: 2^-14 in fp16, which x^ = x rstd of an fp16 x near 1e-4 reaches)
HALF_DENORMAL = {torch.float32: 2.0**-150, torch.float16: 2.0**-25, torch.bfloat16: 2.0**-134}
ids = lambda d: str(d).split('.')[-1] if isinstance(d, torch.dtype) else None


def inputs(rows, width, dtype, salt=0, kind='normal'):
    g = torch.Generator().manual_seed(1000 * width + rows + salt)
    x = 3 + 2 * torch.randn(rows, width, generator=g) if kind == 'normal' else 1000 + torch.randn(rows, width, generator=g)
    gamma = 1 + 0.5 * torch.randn(width, generator=g)
    return x.to(dtype), gamma.to(dtype)


def reference64(x, gamma):
    """float64 on the host from the stored values: rstd, x^, y"""
    x = x.double().cpu()
    rstd = 1.0 / torch.sqrt(x.square().mean(dim=1, keepdim=True) + EPS32)
    xhat = x * rstd
    return rstd, xhat, xhat * (1.0 if gamma is None else gamma.double().cpu())


def plain_fp32(x):
    """the same formulas as plain fp32 torch ops on the GPU: (x^, rstd)"""
    x = x.float()
    rstd = 1.0 / torch.sqrt(x.square().mean(dim=1, keepdim=True) + EPS32)
    return (x * rstd).double().cpu(), rstd.double().cpu()


def run_forward(x, gamma, bits, seed, off, keep=True, want_xhat=True):
    """the call into guarded buffers -> (y, rstd, state, xhat) as Guarded (state / xhat: None when not asked for), after the guards were checked"""
    rows, width = x.shape
    gx = Guarded(x.numel(), x.dtype, off, x)
    gg = None if gamma is None else Guarded(width, x.dtype, off, gamma)
    y, rstd = Guarded(x.numel(), x.dtype, off), Guarded(rows, torch.float32, off)
    state = Guarded(cabi_x.norm_state_bytes(rows, width, bits), torch.uint8, 8 * off) if keep else None
    xhat = Guarded(x.numel(), torch.float32, off) if want_xhat else None
    cabi_x.rms_norm_forward(gx.t.view(rows, width), None if gg is None else gg.t, EPS, bits, seed, keep=keep, y=y.t.view(rows, width), rstd=rstd.t,
                            state=None if state is None else state.t, xhat=None if xhat is None else xhat.t.view(rows, width))
    torch.cuda.synchronize()
    for name, buffer in (('y', y), ('rstd', rstd), ('state', state), ('xhat', xhat)):
        assert buffer is None or buffer.intact(), f'{name}: guard bytes were written'
    for name, buffer in (('x', gx), ('gamma', gg)):
        assert buffer is None or buffer.unchanged(), f'{name} was written'
    return y, rstd, state, xhat


def check_forward_values(x, gamma, y, rstd, xhat, label):
    """x^, rstd and y against float64 by the bounds of the module docstring -> (K of x^, K of rstd, their reference values, torch's y in bounds)"""
    rows, width = x.shape
    rstd64, xhat64, y64 = reference64(x, gamma)
    unit = 2.0**-24 * xhat64.abs() + TINY
    ref_xhat, ref_rstd = plain_fp32(x.to(DEV))
    k_ref = float(((ref_xhat - xhat64).abs() / unit).max())
    k_ref_rstd = float(((ref_rstd - rstd64).abs() / (2.0**-24 * rstd64)).max())
    k = float(((xhat.double().cpu() - xhat64).abs() / unit).max())
    k_rstd = float(((rstd.double().cpu().view(-1, 1) - rstd64).abs() / (2.0**-24 * rstd64)).max())
    allowed = allowance(max(k_ref, k_ref_rstd), width)
    assert k <= allowed and k_rstd <= allowed, f'{label}: K = {k:.2f}, K(rstd) = {k_rstd:.2f}; allowed {allowed:.2f} (plain fp32 ops: {k_ref:.2f}, {k_ref_rstd:.2f})'
    bound = (UNIT[x.dtype] * y64.abs()).clamp_min(HALF_DENORMAL[x.dtype]) + allowed * unit * (1.0 if gamma is None else gamma.double().cpu().abs())
    theirs = F.rms_norm(x.to(DEV), (width, ), None if gamma is None else gamma.to(DEV), EPS)
    torch_in_bounds = float(((theirs.double().cpu() - y64).abs() / bound).max())
    if x.dtype == torch.float32:
        assert torch_in_bounds <= 1.0, f'{label}: torch\'s rms_norm is {torch_in_bounds:.3f} bounds off'
    worst = float(((y.double().cpu() - y64).abs() / bound).max())
    assert worst <= 1.0, f'{label}: y is {worst:.3f} bounds off'
    return k, k_rstd, k_ref, k_ref_rstd, torch_in_bounds


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('dtype', DTYPES, ids=ids)
def test_forward_state_values_and_guards(dtype, bits):
    worst = [0.0] * 5
    for i, (width, rows) in enumerate(itertools.product(WIDTHS, ROWS)):
        off, affine, device_word = options(i)
        x, gamma = inputs(rows, width, dtype)
        gamma = gamma if affine else None
        label = f'{rows} x {width} off {off} affine {affine} device word {device_word}'
        y, rstd, state, xhat = run_forward(x, gamma, bits, seed_argument(device_word), off)
        # the state, bit for bit, from the x^ the kernel quantized
        want = cabi_x.norm_state_host(xhat.t.view(rows, width).cpu(), SEED, bits)
        got = state.t.cpu()
        assert torch.equal(got, want), f'{label}: state differs at bytes {torch.nonzero(got != want).flatten()[:8].tolist()}'
        ks = check_forward_values(x, gamma, y.t.view(rows, width), rstd.t, xhat.t.view(rows, width), label)
        worst = [max(a, b) for a, b in zip(worst, ks)]
        # the plain forward: the same y and rstd bytes, nothing else
        y0, rstd0, _, _ = run_forward(x, gamma, bits, SEED, off, keep=False, want_xhat=False)
        assert torch.equal(y0.raw, y.raw) and torch.equal(rstd0.raw, rstd.raw), label
        # the same arguments, the same bytes
        again = run_forward(x, gamma, bits, SEED, off)
        assert all(torch.equal(a.raw, b.raw) for a, b in zip(again, (y, rstd, state, xhat))), label
    print(f'{dtype} bits {bits}: K(x^) = {worst[0]:.2f}, K(rstd) = {worst[1]:.2f}; plain fp32 torch ops: {worst[2]:.2f}, {worst[3]:.2f}; '
          f'F.rms_norm: {worst[4]:.3f} of the bound of y')


def backward_problem(rows, width, dtype, bits, affine, salt=0):
    g = torch.Generator().manual_seed(7000 * width + rows + salt)
    xhat = torch.randn(rows, width, generator=g)
    state = cabi_x.norm_state_host(xhat, SEED + salt, bits)
    xq = cabi_x.norm_state_unpack_host(state, rows, width, bits)
    rstd = 0.25 + torch.rand(rows, generator=g)
    gy = torch.randn(rows, width, generator=g).to(dtype)
    gamma = (1 + 0.5 * torch.randn(width, generator=g)).to(dtype) if affine else None
    return state, xq, rstd, gy, gamma


def run_backward(state, rstd, gy, gamma, bits, off, want=(True, True), workspace=None):
    rows, width = gy.shape
    g_gy, g_state, g_rstd = Guarded(gy.numel(), gy.dtype, off, gy), Guarded(state.numel(), torch.uint8, 8 * off, state), Guarded(rows, torch.float32, off, rstd)
    g_gamma = None if gamma is None else Guarded(width, gy.dtype, off, gamma)
    dx = Guarded(gy.numel(), gy.dtype, off) if want[0] else None
    dgamma = Guarded(width, torch.float32, off) if want[1] else None
    cabi_x.rms_norm_backward(g_gy.t.view(rows, width), g_state.t, g_rstd.t, None if g_gamma is None else g_gamma.t, bits, want,
                             dx=None if dx is None else dx.t.view(rows, width), dgamma=None if dgamma is None else dgamma.t, workspace=workspace)
    torch.cuda.synchronize()
    for name, buffer in (('dx', dx), ('dgamma', dgamma)):
        assert buffer is None or buffer.intact(), f'{name}: guard bytes were written'
    for name, buffer in (('gy', g_gy), ('state', g_state), ('rstd', g_rstd), ('gamma', g_gamma)):
        assert buffer is None or buffer.unchanged(), f'{name} was written'
    return dx, dgamma


def check_backward_values(xq, rstd, gy, gamma, dx, dgamma, label):
    rows, width = gy.shape
    gy64, xq64, rstd64 = gy.double(), xq.double(), rstd.double().view(-1, 1)
    gh = gy64 * (1.0 if gamma is None else gamma.double())
    dx64 = rstd64 * (gh - xq64 * (gh * xq64).mean(dim=1, keepdim=True))
    unit = 2.0**-24 * rstd64 * (gh.abs() + xq64.abs() * (gh * xq64).abs().mean(dim=1, keepdim=True))
    # plain fp32 torch ops on the GPU for the same formula
    g32 = gy.to(DEV).float() * (1.0 if gamma is None else gamma.to(DEV).float())
    q32, r32 = xq.to(DEV), rstd.to(DEV).view(-1, 1)
    ref = (r32 * (g32 - q32 * (g32 * q32).mean(dim=1, keepdim=True))).double().cpu()
    k_ref = float(((ref - dx64).abs() / unit).max())
    allowed = allowance(k_ref, width)
    err = (dx.double().cpu() - dx64).abs()
    k = float(((err - (UNIT[gy.dtype] * dx64.abs()).clamp_min(HALF_DENORMAL[gy.dtype])).clamp_min(0) / unit).max())
    assert k <= allowed, f"{label}: K' = {k:.2f}, allowed {allowed:.2f} (plain fp32 ops: {k_ref:.2f})"
    terms = gy64 * xq64
    assert bool(((dgamma.double().cpu() - terms.sum(dim=0)).abs() <= (rows + 3) * 2.0**-24 * terms.abs().sum(dim=0)).all()), f'{label}: dgamma'
    return k, k_ref


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('dtype', DTYPES, ids=ids)
def test_backward_from_a_given_state(dtype, bits):
    worst = [0.0, 0.0]
    for i, (width, rows) in enumerate(itertools.product(WIDTHS, ROWS)):
        off, affine, _ = options(i)
        state, xq, rstd, gy, gamma = backward_problem(rows, width, dtype, bits, affine)
        label = f'{rows} x {width} off {off} affine {affine}'
        dx, dgamma = run_backward(state, rstd, gy, gamma, bits, off)
        ks = check_backward_values(xq, rstd, gy, gamma, dx.t.view(rows, width), dgamma.t, label)
        worst = [max(a, b) for a, b in zip(worst, ks)]
        again = run_backward(state, rstd, gy, gamma, bits, off)
        assert all(torch.equal(a.raw, b.raw) for a, b in zip(again, (dx, dgamma))), f'{label}: two runs differ'
        # NULL outputs are skipped: the other keeps its bytes, and without dgamma the workspace is not touched
        scratch = torch.full((cabi_x.norm_workspace_bytes(rows, width), ), FILL, dtype=torch.uint8, device=DEV)
        only_dx, none_g = run_backward(state, rstd, gy, gamma, bits, off, (True, False), scratch)
        assert none_g is None and torch.equal(only_dx.raw, dx.raw) and bool((scratch == FILL).all()), label
        none_dx, only_g = run_backward(state, rstd, gy, gamma, bits, off, (False, True))
        assert none_dx is None and torch.equal(only_g.raw, dgamma.raw), label
    print(f"{dtype} bits {bits}: K'(dx) = {worst[0]:.2f}; plain fp32 torch ops: {worst[1]:.2f}")


@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16), ids=ids)
def test_width_8_one_row_past_a_full_sweep_of_the_grid(dtype):
    """32 rows of width 8 share a forward workgroup, 128 a backward one: forward sweeps 16384 * 32 rows at once, backward 512 * 128; one row more
    than the longer sweep starts the next one of both"""
    rows, width, bits = 16384 * 32 + 1, 8, 4
    x, gamma = inputs(rows, width, dtype)
    y, rstd, state, xhat = run_forward(x, gamma, bits, SEED, 0)
    assert torch.equal(state.t.cpu(), cabi_x.norm_state_host(xhat.t.view(rows, width).cpu(), SEED, bits))
    check_forward_values(x, gamma, y.t.view(rows, width), rstd.t, xhat.t.view(rows, width), 'the long sweep')
    host_state, xq, rstd_given, gy, gamma = backward_problem(rows, width, dtype, bits, True)
    dx, dgamma = run_backward(host_state, rstd_given, gy, gamma, bits, 1)
    check_backward_values(xq, rstd_given, gy, gamma, dx.t.view(rows, width), dgamma.t, 'the long sweep')


@pytest.mark.parametrize('rows', (4097, 2 * 4096 + 1), ids=('second_tile', 'third_tile'))
def test_backward_width_520_a_workgroup_walks_on_with_one_row_sum_through_lds(rows):
    """128 lanes per row, 8 rows per tile, 512 workgroups: with 4097 rows workgroup 0 walks a second tile, with 8193 a third -- the tile whose
    row sum writes the slots of the first again"""
    width, bits, dtype = 520, 4, torch.float32
    state, xq, rstd, gy, gamma = backward_problem(rows, width, dtype, bits, True)
    dx, dgamma = run_backward(state, rstd, gy, gamma, bits, 0)
    k = check_backward_values(xq, rstd, gy, gamma, dx.t.view(rows, width), dgamma.t, f'{rows} x {width}')
    again = run_backward(state, rstd, gy, gamma, bits, 0)
    assert all(torch.equal(a.raw, b.raw) for a, b in zip(again, (dx, dgamma)))
    print(f"{rows} x {width}: K'(dx) = {k[0]:.2f}; plain fp32 torch ops: {k[1]:.2f}")


@pytest.mark.parametrize('rows', (2 * 16384 + 1, 4 * 16384 + 1), ids=('second_tile', 'third_tile'))
def test_forward_width_520_a_workgroup_walks_on_with_one_row_sum_through_lds(rows):
    """128 lanes per row, 2 rows per tile, 16384 workgroups, bf16: workgroup 0 walks a second tile, and with 4 * 16384 + 1 rows a third"""
    width, bits, dtype = 520, 4, torch.bfloat16
    x, gamma = inputs(rows, width, dtype)
    y, rstd, state, xhat = run_forward(x, gamma, bits, SEED, 0)
    assert torch.equal(state.t.cpu(), cabi_x.norm_state_host(xhat.t.view(rows, width).cpu(), SEED, bits))
    k = check_forward_values(x, gamma, y.t.view(rows, width), rstd.t, xhat.t.view(rows, width), f'{rows} x {width}')
    again = run_forward(x, gamma, bits, SEED, 0)
    assert all(torch.equal(a.raw, b.raw) for a, b in zip(again, (y, rstd, state, xhat)))
    print(f'{rows} x {width}: K(x^) = {k[0]:.2f}, K(rstd) = {k[1]:.2f}; plain fp32 torch ops: {k[2]:.2f}, {k[3]:.2f}')


@pytest.mark.parametrize('case', walks('backward', 1), ids=str)
def test_backward_a_workgroup_walks_on_at_every_lanes_per_row(case):
    """16 to 1024 lanes per row, 512 workgroups (asserted from the workspace query): one row past one and past two sweeps -- workgroup 0 alone walks on,
    with one live row in a tile of dead lanes; on its third tile the ONE row sum of 4, 8 or 16 waves writes the slots of the first again -- and three
    full sweeps.  The column accumulators are carried across the tiles into the direct store (1 row per tile), the LDS column loop (2 or 4 rows
    per tile: more than one trip) or the plain one, and 512 partials per column enter the column sums"""
    backward_walks_on(case, backward_problem, run_backward, check_backward_values)


@pytest.mark.parametrize('case', walks('forward', 1), ids=str)
def test_forward_a_workgroup_walks_on_at_every_lanes_per_row(case):
    """16 to 256 lanes per row and 1, 2 or 4 blocks per lane, one row past one or two sweeps of the 16384 workgroups (norm_harness.forward_walks_on)"""
    forward_walks_on(case, inputs, run_forward, check_forward_values)


@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16), ids=ids)
def test_a_finite_row_whose_sum_of_squares_overflows_gives_rstd_0_and_zeros(dtype):
    """The header: "a finite row whose fp32 sum of squares overflows gives rstd = 0 and x^ = y = +-0".  One row of values of either sign and of
    size 2^66 .. 2^67 among ordinary rows: rstd = 0, x^ and y are zeros, no group is poisoned (the host decode is 0, not NaN); backward from that
    state: dx of the row is 0, dgamma is finite and the bytes of the same call without the row's gy.  Every other row has the bytes of a run where
    the row holds ordinary values"""
    rows, width, bits, at = 5, 200, 4, 2
    clean, gamma = inputs(rows, width, dtype, 5)
    g = torch.Generator().manual_seed(9)
    x = clean.clone()
    x[at] = (2.0**66 * (1 + torch.rand(width, generator=g)) * (1 - 2 * torch.randint(0, 2, (width, ), generator=g))).to(dtype)
    gy = torch.randn(rows, width, generator=g).to(dtype)
    others = [r for r in range(rows) if r != at]
    assert bool(torch.isfinite(x).all()) and bool(torch.isinf(x[at].float().square().sum()))
    y, rstd, state, xhat = run_forward(x, gamma, bits, SEED, 0)
    y0, rstd0, state0, xhat0 = run_forward(clean, gamma, bits, SEED, 0)
    assert float(rstd.t[at]) == 0.0 and not bool(xhat.t.view(rows, width)[at].any()) and not bool(y.t.view(rows, width)[at].any())
    xq = cabi_x.norm_state_unpack_host(state.t.cpu(), rows, width, bits)
    assert not bool(torch.isnan(xq).any()) and not bool(xq[at].any())
    assert all(torch.equal(a[others], b[others]) for a, b in zip(state_rows(state.t, rows, width), state_rows(state0.t, rows, width)))
    for a, b in ((y, y0), (xhat, xhat0), (rstd, rstd0)):
        assert torch.equal(a.t.view(rows, -1)[others].view(torch.uint8), b.t.view(rows, -1)[others].view(torch.uint8))
    dx, dgamma = run_backward(state.t, rstd.t, gy, gamma, bits, 0)
    dx0 = run_backward(state0.t, rstd0.t, gy, gamma, bits, 0)[0]
    assert not bool(dx.t.view(rows, width)[at].any()) and torch.equal(dx.t.view(rows, width)[others], dx0.t.view(rows, width)[others])
    without = gy.clone()
    without[at] = 0
    assert bool(torch.isfinite(dgamma.t).all()) and torch.equal(run_backward(state.t, rstd.t, without, gamma, bits, 0)[1].raw, dgamma.raw)


@pytest.mark.parametrize('bits', BITS)
def test_value_edges(bits):
    rows, width = 6, 200
    # a zero row: x^ = 0, every code 0, y = 0, rstd = 1 / sqrt(float32(eps))
    x = torch.zeros(rows, width)
    y, rstd, state, xhat = run_forward(x, None, bits, SEED, 0)
    assert not bool(xhat.t.any()) and not bool(state.t.any()) and not bool(y.t.any())
    assert rstd.t.cpu().numpy().tolist() == [float(np.float32(1) / np.sqrt(np.float32(EPS)))] * rows
    # rows of 1000 + N(0, 1) in fp32 stay inside the bound of x^
    x, gamma = inputs(rows, width, torch.float32, kind='offset')
    y, rstd, state, xhat = run_forward(x, gamma, bits, SEED, 1)
    k = check_forward_values(x, gamma, y.t.view(rows, width), rstd.t, xhat.t.view(rows, width), '1000 + N(0, 1)')
    print(f'bits {bits}: rows of 1000 + N(0, 1): K(x^) = {k[0]:.2f}, K(rstd) = {k[1]:.2f}; plain fp32 torch ops: {k[2]:.2f}, {k[3]:.2f}')
    # denormal rows give no NaN
    tiny = (torch.randn(rows, width) * 1e-40).float()
    y, rstd, state, xhat = run_forward(tiny, gamma, bits, SEED, 0)
    assert not bool(torch.isnan(y.t).any()) and not bool(torch.isnan(xhat.t).any()) and not bool(torch.isnan(rstd.t).any())
    assert not bool(torch.isnan(cabi_x.norm_state_unpack_host(state.t.cpu(), rows, width, bits)).any())


@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16), ids=ids)
@pytest.mark.parametrize('poison', ('nan', 'inf'))
def test_a_non_finite_element_gives_the_patterns_of_the_definition_and_touches_no_other_row(poison, dtype):
    rows, width, bits, at = 5, 200, 4, 77
    clean, gamma = inputs(rows, width, dtype, 3)
    x = clean.clone()
    x[2, at] = float(poison)
    gy = torch.randn(rows, width).to(dtype)
    results = []
    for source in (clean, x):
        y, rstd, state, xhat = run_forward(source, gamma, bits, SEED, 0)
        dx, dgamma = run_backward(state.t, rstd.t, gy, gamma, bits, 0)
        results.append((y.t.view(rows, width).cpu(), dx.t.view(rows, width).cpu(), dgamma.t.cpu(), xhat.t.view(rows, width).cpu(), rstd.t.cpu(),
                        cabi_x.norm_state_unpack_host(state.t.cpu(), rows, width, bits)))
    (y0, dx0, dgamma0, _, rstd0, _), (y1, dx1, dgamma1, xhat1, rstd1, xq1) = results
    others = [0, 1, 3, 4]
    group = torch.zeros(width, dtype=torch.bool)
    group[at // 64 * 64:at // 64 * 64 + 64] = True                      # the columns of the group that holds the element
    assert bool(torch.isnan(dx1[2]).all()) and not bool(torch.isnan(dgamma0).any())
    if poison == 'nan':                                                 # the whole row of x^ and y, every group of it, every column of dgamma
        assert bool(torch.isnan(xhat1[2]).all()) and bool(torch.isnan(y1[2]).all()) and bool(torch.isnan(xq1[2]).all()) and bool(torch.isnan(rstd1[2]))
        assert bool(torch.isnan(dgamma1).all())
    else:                                                               # rstd = 0: x^ is NaN at the element and +-0 elsewhere; its group is poisoned
        here = torch.zeros(width, dtype=torch.bool)
        here[at] = True
        assert float(rstd1[2]) == 0.0 and bool(torch.isnan(xhat1[2, at])) and not bool(xhat1[2, ~here].any())
        assert bool(torch.isnan(y1[2, at])) and not bool(y1[2, ~here].any())
        assert bool(torch.isnan(xq1[2, group]).all()) and not bool(xq1[2, ~group].any())
        assert bool(torch.isnan(dgamma1[group]).all()) and not bool(torch.isnan(dgamma1[~group]).any())
        theirs = F.rms_norm(x.to(DEV), (width, ), gamma.to(DEV), EPS)
        assert torch.equal(torch.isnan(theirs).cpu(), torch.isnan(y1))       # elementwise NaN-ness as torch's own formulation
    assert torch.equal(y1[others], y0[others]) and torch.equal(dx1[others], dx0[others]) and torch.equal(rstd1[others], rstd0[others])
