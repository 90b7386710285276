"""The moments of the variance estimator on the GPU (fewbit_amd/csrc/fewbit_moments.hip through cabi_x.row_moments / sum_squares, and
fewbit_amd.variance on top of them), against float64 on the host.

The kernel's plan (a pure function of the row count): a workgroup of 4 waves serves ``per = max(16, ceil(rows / 1024))`` consecutive rows,
there are ``ceil(rows / per) <= 1024`` workgroups, and a second launch adds their partials.  ``sum_squares`` cuts its array into pieces of
1024 elements and deals them like rows, at least 4 to a workgroup.  Hence the boundaries visited below: rows 16 | 17 and 32 | 33 (one more
workgroup), 16383 | 16384 | 16385 (1024 workgroups of 16 rows: the cap is reached; then 964 of 17), 17408 | 17409 (1024 of 17; then 18);
counts 1024 | 1025, 4096 | 4097 and 4194304 | 4194305 (1024 workgroups of 4 pieces; then 5).
"""
import math

import pytest
import torch

import fewbit_amd as fewbit
from fewbit_amd import cabi_x, variance

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
PAIRS = [(dx, dg) for dx in DTYPES for dg in DTYPES]
NAME = lambda dt: str(dt).replace('torch.', '')                      # noqa: E731
PAIR_IDS = [f'{NAME(dx)}-{NAME(dg)}' for dx, dg in PAIRS]
WORKSPACE = 1024 * 3 * 8

ROWS = (1, 2, 3, 63, 64, 65, 255, 257, 1000)
SHAPES = ((1, 1), (7, 9), (8, 8), (15, 17), (64, 64), (65, 63), (200, 770), (770, 200), (1024, 8))
PLAN_ROWS = (16, 17, 32, 33, 16383, 16384, 16385, 17408, 17409)
COUNTS = (1, 7, 8, 9, 255, 256, 257, 65537, 770 * 3072)
PLAN_COUNTS = (1024, 1025, 4096, 4097, 4194304, 4194305)


# ---- shared data and float64 references, computed once on the host ---------------------------------------------------------------------
class _Ints:
    """integer-valued entries in [-3, 3] (exact in every dtype) and the float64 moments of any leading block of them"""

    def __init__(self):
        gen = torch.Generator().manual_seed(2201)
        self.x = torch.randint(-3, 4, (1000, 1024), generator=gen).double()
        self.g = torch.randint(-3, 4, (1000, 1024), generator=gen).double()
        self.tall_x = torch.randint(-3, 4, (17409, 7), generator=gen).double()
        self.tall_g = torch.randint(-3, 4, (17409, 9), generator=gen).double()
        self.flat = torch.randint(-3, 4, (4194305, ), generator=gen).double()
        self.flat_prefix = torch.cumsum(self.flat * self.flat, 0)      # integers below 2^53: exact
        self.cache = {}

    def moments(self, x, g):
        xx, gg = (x * x).sum(1), (g * g).sum(1)
        return torch.stack((xx.sum(), gg.sum(), (xx * gg).sum()))          # every partial sum an integer below 2^53: exact in any order

    def case(self, rows, n, m, tall=False):
        key = (rows, n, m, tall)
        if key not in self.cache:
            x, g = (self.tall_x, self.tall_g) if tall else (self.x, self.g)
            x, g = x[:rows, :n], g[:rows, :m]
            self.cache[key] = (x, g, self.moments(x, g))
        return self.cache[key]


@pytest.fixture(scope='module')
def ints():
    return _Ints()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def same_bits(got, want):
    return torch.equal(bits(got), bits(want.to(torch.float64)))


def nan_workspace():
    return torch.full((WORKSPACE // 8, ), float('nan'), dtype=torch.float64, device=DEV).view(torch.uint8)


# ---- 1. exactness ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dx,dg', PAIRS, ids=PAIR_IDS)
def test_row_moments_is_exact_on_small_integers(ints, dx, dg):
    """Integer entries in [-3, 3]: every square, row sum, product and partial sum is an integer below 2^53, so the three doubles equal the
    host's float64 values bit for bit -- at every contiguous shape of the list and on either side of each boundary of the plan."""
    cases = [(rows, n, m, False) for rows in ROWS for n, m in SHAPES] + [(rows, 7, 9, True) for rows in PLAN_ROWS]
    bad = []
    for rows, n, m, tall in cases:
        x, g, want = ints.case(rows, n, m, tall)
        got = cabi_x.row_moments(x.to(DEV).to(dx), g.to(DEV).to(dg))
        assert got.dtype == torch.float64 and got.shape == (3, ) and got.device.type == 'cuda'
        if not same_bits(got, want):
            bad.append((rows, n, m, got.tolist(), want.tolist()))
    assert not bad, bad[:5]


@pytest.mark.parametrize('dtype', DTYPES, ids=NAME)
def test_sum_squares_is_exact_on_small_integers(ints, dtype):
    bad = []
    for count in COUNTS + PLAN_COUNTS:
        got = cabi_x.sum_squares(ints.flat[:count].to(DEV).to(dtype))
        assert got.dtype == torch.float64 and got.shape == (1, )
        if not same_bits(got, ints.flat_prefix[count - 1:count]):
            bad.append((count, got.tolist(), float(ints.flat_prefix[count - 1])))
    assert not bad, bad
    # any shape counts as its elements
    t = ints.flat[:770 * 64].reshape(770, 64).to(DEV).to(dtype)
    assert same_bits(cabi_x.sum_squares(t), ints.flat_prefix[770 * 64 - 1:770 * 64])


# ---- 2. alignment and bounds ----------------------------------------------------------------------------------------------------------
def _views(data, dtype):
    """``data`` (float64, rows x n) as views of NaN-filled allocations: ld = n + 1, ld = 2 n (both halves of a chunk), and base pointers
    shifted by 1 .. 7 elements; a NaN row before and after inside the same allocation"""
    rows, n = data.shape
    data = data.to(DEV).to(dtype)

    def inside(width, start):
        buf = torch.full((rows + 2, width), float('nan'), dtype=dtype, device=DEV)
        view = buf[1:rows + 1, start:start + n]
        view.copy_(data)
        return view

    out = [('ld = n + 1', inside(n + 1, 0))]
    for half in (0, 1):
        buf = torch.full((rows + 2, 2 * n), float('nan'), dtype=dtype, device=DEV)
        view = buf[1:rows + 1].chunk(2, -1)[half]
        view.copy_(data)
        out.append((f'chunk {half}', view))
    out += [(f'shift {s}', inside(n + 8, s)) for s in range(1, 8)]
    return out


@pytest.mark.parametrize('dx,dg', PAIRS, ids=PAIR_IDS)
def test_strided_and_shifted_rows_read_nothing_but_their_elements(ints, dx, dg):
    """Everything outside the viewed elements is NaN -- the padding of every row, the rows before and after in the same allocation, the
    workspace: one stray read would show.  The results are those of the contiguous call, bit for bit (and exact: integer data)."""
    bad = []
    for rows in (3, 65):
        for n, m in ((7, 9), (65, 63), (200, 770)):
            x, g, want = ints.case(rows, n, m)
            plain = cabi_x.row_moments(x.to(DEV).to(dx), g.to(DEV).to(dg))
            assert same_bits(plain, want)
            for (how_x, vx), (how_g, vg) in zip(_views(x, dx), _views(g, dg)):
                assert cabi_x._rows_of(vx, 'x') is vx and cabi_x._rows_of(vg, 'g') is vg and not vx.is_contiguous()      # taken as they are, no copy
                got = cabi_x.row_moments(vx, vg, workspace=nan_workspace())
                mixed = cabi_x.row_moments(vx, g.to(DEV).to(dg), workspace=nan_workspace())
                if not (same_bits(got, plain) and same_bits(mixed, plain)) or bool(torch.isnan(got).any()):
                    bad.append((rows, n, m, how_x, got.tolist(), plain.tolist()))
    assert not bad, bad[:5]


@pytest.mark.parametrize('dtype', DTYPES, ids=NAME)
def test_sum_squares_at_any_base_offset_reads_only_its_elements(ints, dtype):
    bad = []
    for count in (1, 9, 257, 5000):
        for shift in range(0, 8):
            buf = torch.full((count + 16, ), float('nan'), dtype=dtype, device=DEV)
            view = buf[shift:shift + count]
            view.copy_(ints.flat[:count].to(DEV).to(dtype))
            got = cabi_x.sum_squares(view, workspace=nan_workspace())
            if not same_bits(got, ints.flat_prefix[count - 1:count]):
                bad.append((count, shift, got.tolist()))
    assert not bad, bad[:5]


def test_other_layouts_are_made_contiguous_and_outputs_can_be_passed(ints):
    x, g, want = ints.case(65, 15, 17)
    xt = x.T.contiguous().to(DEV).bfloat16().T                       # unit stride along the rows: copied
    gs = g.to(DEV).float().repeat_interleave(2, dim=1)[:, ::2]       # stride 2 along the columns: copied
    assert xt.stride(1) != 1 and gs.stride(1) == 2
    out, ws = torch.full((3, ), float('nan'), dtype=torch.float64, device=DEV), nan_workspace()
    assert cabi_x.row_moments(xt, gs, out=out, workspace=ws) is out and same_bits(out, want)
    with pytest.raises(cabi_x.FewbitHipError, match='out must be'):
        cabi_x.row_moments(xt, gs, out=torch.empty(3, device=DEV))
    with pytest.raises(cabi_x.FewbitHipError, match='same number of rows'):
        cabi_x.row_moments(xt, gs[:64])
    with pytest.raises(cabi_x.FewbitHipError, match='rows = 0'):
        cabi_x.row_moments(xt.contiguous()[:0], gs.contiguous()[:0])


# ---- 3. random data -------------------------------------------------------------------------------------------------------------------
def _fsum_moments(x, g):
    """the exact (correctly rounded) sums of the float64 squares, row by row and over the rows; the products are rounded once"""
    xs, gs = (x.double().cpu().numpy())**2, (g.double().cpu().numpy())**2          # exact: the operands have at most 24 significant bits
    xx, gg = [math.fsum(r) for r in xs], [math.fsum(r) for r in gs]
    return math.fsum(xx), math.fsum(gg), math.fsum(a * b for a, b in zip(xx, gg))


def _close(got, want, rel):
    if math.isinf(want) or math.isnan(want):
        return got == want or (math.isnan(got) and math.isnan(want))
    return abs(got - want) <= rel * abs(want)


@pytest.mark.parametrize('dx,dg', PAIRS, ids=PAIR_IDS)
def test_random_rows_are_within_the_fp64_summation_bound(dx, dg):
    """randn scaled by 2^+20 and 2^-20 (crosswise): 257 x (200, 770).  Every output is a sum of at most rows * max(n, m) exactly squared terms
    (and, for sxg, one rounded product per row) added in fp64: within rows * max(n, m) * 2^-53 relative of the exact value, whatever the order.
    (2^20 randn overflows fp16 to Inf, 2^-20 randn are fp16 subnormals: the reference is taken of the operands as rounded, Inf included.)
    Two identical calls give identical bits."""
    rows, n, m = 257, 200, 770
    rel = rows * max(n, m) * 2.0**-53
    gen = torch.Generator().manual_seed(7)
    for ex, eg in ((20, -20), (-20, 20)):
        x = (torch.randn(rows, n, generator=gen) * 2.0**ex).to(dx).to(DEV)
        g = (torch.randn(rows, m, generator=gen) * 2.0**eg).to(dg).to(DEV)
        got = cabi_x.row_moments(x, g)
        again = cabi_x.row_moments(x.clone(), g.clone())
        assert torch.equal(bits(got), bits(again))
        want = _fsum_moments(x, g)
        print(f'row_moments {NAME(dx)} x 2^{ex}, {NAME(dg)} x 2^{eg}: got {got.tolist()}, exact {want}, bound {rel:.3e}')
        for k in range(3):
            assert _close(float(got[k]), want[k], rel), (k, float(got[k]), want[k])
        t = x.T.contiguous()
        one = cabi_x.sum_squares(t)
        assert torch.equal(bits(one), bits(cabi_x.sum_squares(t.clone())))
        assert _close(float(one), want[0], rows * n * 2.0**-53), (float(one), want[0])


def test_the_largest_bf16_values_do_not_overflow():
    x = torch.full((4, 16), 3e38, dtype=torch.bfloat16, device=DEV)
    g = torch.full((4, 24), -3e38, dtype=torch.bfloat16, device=DEV)
    v = float(x[0, 0].double())**2
    got = cabi_x.row_moments(x, g)
    assert bool(torch.isfinite(got).all())
    assert same_bits(got, torch.tensor([64 * v, 96 * v, 4 * (16 * v) * (24 * v)], dtype=torch.float64))
    assert same_bits(cabi_x.sum_squares(x), torch.tensor([64 * v], dtype=torch.float64))
    big = torch.full((4, 16), 3e38, dtype=torch.float32, device=DEV)
    assert same_bits(cabi_x.row_moments(big, g)[:1], torch.tensor([64 * float(big[0, 0].double())**2], dtype=torch.float64))


@pytest.mark.parametrize('dx,dg', ((torch.float32, torch.bfloat16), (torch.float16, torch.float32), (torch.bfloat16, torch.float16)), ids=NAME)
def test_nan_and_inf_reach_the_outputs_they_belong_to_and_no_other(dx, dg):
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(65, 63, generator=gen).to(dx).to(DEV)
    g = torch.randn(65, 65, generator=gen).to(dg).to(DEV)
    clean = cabi_x.row_moments(x, g)
    assert bool(torch.isfinite(clean).all())
    xn = x.clone()
    xn[40, 62] = float('nan')
    got = cabi_x.row_moments(xn, g)
    assert math.isnan(float(got[0])) and math.isnan(float(got[2])) and torch.equal(bits(got[1:2]), bits(clean[1:2]))
    gi = g.clone()
    gi[7, 0] = float('-inf')
    got = cabi_x.row_moments(x, gi)
    assert float(got[1]) == math.inf and float(got[2]) == math.inf and torch.equal(bits(got[0:1]), bits(clean[0:1]))
    assert math.isnan(float(cabi_x.sum_squares(xn))) and float(cabi_x.sum_squares(gi)) == math.inf


# ---- 4. the estimator end to end ---------------------------------------------------------------------------------------------------------
B, N_IN, N_OUT = 256, 64, 96


def _float64_triple(x, g, bs, bs_proj, gemm_dtype=None):
    """the three formulas in float64 on the host, with the bound on each that follows from |d cross| <= 2 B 2^-24 sqrt(cross sx sg) (fp32
    accumulation of B products per entry of the GEMM, then Cauchy-Schwarz over the entries; ``exact``: no GEMM error at all), the fp64
    summation bound of the kernels, and one rounding to fp32 of the result (2^-23 relative, which also covers the fp64 formula arithmetic).
    ``gemm_dtype``: the operands are rounded to it for cross alone (the mixed-dtype contract)."""
    x, g = x.detach().cpu(), g.detach().cpu()
    xd, gd = x.double(), g.double()
    xx, gg = (xd * xd).sum(1), (gd * gd).sum(1)
    sx, sg, sxg = float(xx.sum()), float(gg.sum()), float(xx @ gg)
    xr, gr = (xd, gd) if gemm_dtype is None else (x.to(gemm_dtype).double(), g.to(gemm_dtype).double())
    cross = float(((xr.T @ gr)**2).sum())
    return (sx, sg, sxg, cross), (cross / (sx * sg), sxg * (bs / (bs - 1)) - cross / (bs - 1), (sx * sg - cross) / bs_proj)


def _check_triple(got, x, g, bs, bs_proj, exact, what, gemm_dtype=None):
    (sx, sg, sxg, cross), want = _float64_triple(x, g, bs, bs_proj, gemm_dtype)
    d_cross = 0.0 if exact else 2 * bs * 2.0**-24 * math.sqrt(cross * sx * sg)
    d_sum = bs * max(x.shape[-1], g.shape[-1]) * 2.0**-53            # relative, of sx, sg, sxg (and count * 2^-53 <= this for cross: n m <= B max)
    d_sum = max(d_sum, x.shape[-1] * g.shape[-1] * 2.0**-53)
    bounds = (d_cross / (sx * sg) + 3 * d_sum * want[0], d_cross / (bs - 1) + d_sum * (sxg * bs / (bs - 1) + cross / (bs - 1)),
              (d_cross + d_sum * (2 * sx * sg + cross)) / bs_proj)
    for k, name in enumerate(('corr', 'var_sgd', 'var_rmm')):
        assert got[k].dtype == torch.float32 and got[k].dim() == 0 and got[k].device.type == 'cuda'
        err, tol = abs(float(got[k].double()) - want[k]), bounds[k] + 2.0**-23 * abs(want[k])
        print(f'{what}: {name} = {float(got[k]):.9g}, float64 {want[k]:.9g}, error / bound = {err / tol:.4f}')
        assert err <= tol, (what, name, float(got[k]), want[k], err, tol)


def _operands(kind, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind == 'integers':
        x, w = torch.randint(-3, 4, (B, N_IN), generator=gen).float(), torch.randint(-3, 4, (B, N_OUT), generator=gen).float()
    else:
        x, w = torch.randn(B, N_IN, generator=gen), torch.randn(B, N_OUT, generator=gen)
    return x.to(dtype).to(DEV), w.to(DEV)


@pytest.fixture
def seam(monkeypatch):
    calls, real = [], variance._cross_product

    def counted(x, g):
        calls.append((x.dtype, g.dtype))
        out = real(x, g)
        assert out.dtype == torch.float32 and out.shape == (g.shape[1], x.shape[1])
        return out

    monkeypatch.setattr(variance, '_cross_product', counted)
    return calls


@pytest.mark.parametrize('matmul', ('rademacher', 'dct'))
@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float32, torch.float16), ids=NAME)
@pytest.mark.parametrize('kind', ('integers', 'randn'))
def test_the_estimator_on_a_randomized_layer_matches_the_float64_formulas(kind, dtype, matmul, seam):
    """VarianceEstimator(RandomizedLinear(64 -> 96, matmul)) on 256 rows.  The gradient that reaches the layer's output is ``w`` itself (the
    loss is sum(out * w)): integer-valued operands make the GEMM exact (|entries| <= 256 * 9), so the triple is the float64 formulas to one
    fp32 rounding; randn operands get the derived bound of ``_check_triple``."""
    seen = []
    est = fewbit.variance.VarianceEstimator(fewbit.RandomizedLinear(N_IN, N_OUT, proj_dim_ratio=0.25, matmul=matmul, device=DEV, dtype=dtype), lambda *a: seen.append(a))
    assert 'fewbit_hipx_row_moments' in variance.variance_path(torch.empty(B, N_IN, device=DEV, dtype=dtype), torch.empty(B, N_OUT, device=DEV, dtype=dtype))
    for step in range(2):
        x, w = _operands(kind, dtype, 100 + step)
        w = w.to(dtype)
        (est(x) * w).sum().backward()
        assert len(seam) == step + 1 and seam[-1] == (dtype, dtype)                  # one GEMM per backward
        assert torch.equal(est.state.input, x) and est.state.input.dtype == dtype and torch.equal(est.state.grad_output, w)
        assert est.state.step == step + 1 and len(seen) == step + 1 and seen[-1][3] == step and seen[-1][0] is est.variance[0]
        _check_triple(est.variance, x, w, B, B // 4, kind == 'integers', f'{matmul} {NAME(dtype)} {kind} step {step}')
    assert est.state.bs == B and est.state.bs_proj == B // 4


@pytest.mark.parametrize('kind', ('integers', 'randn'))
def test_fp32_input_with_a_bf16_gradient_multiplies_in_bf16(kind, seam):
    """autocast: the layer's input stays fp32, the gradient that reaches its output is bf16.  sx is that of the fp32 input as it is; cross
    is the GEMM of the input rounded to bf16, the precision the layer's own weight-gradient GEMM has there."""
    est = fewbit.variance.VarianceEstimator(fewbit.RandomizedLinear(N_IN, N_OUT, proj_dim_ratio=0.25, matmul='rademacher', device=DEV))
    x, w = _operands(kind, torch.float32, 300)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = est(x)
        assert out.dtype == torch.bfloat16
        (out * w.bfloat16()).sum().backward()
    x_seen, g_seen = est.state.input, est.state.grad_output
    assert x_seen.dtype == torch.float32 and g_seen.dtype == torch.bfloat16 and torch.equal(x_seen, x) and torch.equal(g_seen, w.bfloat16())
    assert len(seam) == 1 and seam[0] == (torch.float32, torch.bfloat16)            # the seam is handed the operands as they are and rounds inside
    _check_triple(est.variance, x_seen, g_seen, B, B // 4, kind == 'integers', f'autocast {kind}', gemm_dtype=torch.bfloat16)
    # the moments themselves: the first three of the operands as they are
    moments = variance.gradient_moments(x_seen, g_seen)
    assert moments.dtype == torch.float64 and moments.shape == (4, ) and torch.equal(bits(moments[:3]), bits(cabi_x.row_moments(x_seen, g_seen)))


def test_the_pytorch_formulation_is_taken_when_the_kernels_are_switched_off(seam):
    x, w = _operands('randn', torch.bfloat16, 400)
    w = w.bfloat16()
    prev = fewbit.linear.use_native_sketch(False)
    try:
        assert 'float64 PyTorch' in variance.variance_path(x, w)
        off = variance.gradient_moments(x, w)
    finally:
        fewbit.linear.use_native_sketch(prev)
    assert not seam and off.device.type == 'cuda' and off.dtype == torch.float64
    on = variance.gradient_moments(x, w)
    assert len(seam) == 1
    rel = B * N_OUT * 2.0**-53 + 2.0**-50                          # (the float64 torch sums have their own rounding)
    assert bool(((on[:3] - off[:3]).abs() <= rel * off[:3]).all())
    sx, sg, cross = float(off[0]), float(off[1]), float(off[3])
    assert abs(float(on[3]) - cross) <= 2 * B * 2.0**-24 * math.sqrt(cross * sx * sg)
    assert 'float64 PyTorch' in variance.variance_path(x.double(), w.double()) and 'float64 PyTorch' in variance.variance_path(x.cpu(), w.cpu())


# ---- 5. transient memory --------------------------------------------------------------------------------------------------------------
def test_postprocess_allocates_the_product_and_the_workspace_and_no_copy_of_the_operands():
    """4096 x 256 / 512 in bf16: the fp32 product (512 KiB), the workspace and 1 MiB of slack (the allocator's rounding, the results).  The
    fp32 copies of the operands alone are 12 MiB."""
    rows, n, m = 4096, 256, 512
    state = variance._VarianceState()
    state.bs, state.bs_proj = rows, rows // 4
    state.input = torch.randn(rows, n, device=DEV).bfloat16()
    state.grad_output = torch.randn(rows, m, device=DEV).bfloat16()
    state.postprocess()                                              # warm-up: the GEMM library's own workspace, the library load
    torch.cuda.synchronize()
    state.variance = None
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    state.postprocess()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    allowed = n * m * 4 + cabi_x.moments_workspace_bytes(rows, n, m) + (1 << 20)
    print(f'postprocess at {rows} x {n} / {m} bf16: peak rise {rise} bytes, allowed {allowed}')
    assert rise <= allowed, (rise, allowed)
    assert state.step == 2 and all(v.dtype == torch.float32 and v.dim() == 0 for v in state.variance)


# ---- 6. hipGraph capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float32), ids=NAME)
def test_an_estimator_without_a_callback_is_captured_with_its_layer(dtype):
    """A training step of the wrapped layer in ONE graph (a read-back or a synchronisation while capturing would fail the capture), replayed
    on two input fills: ``.variance`` follows the fill and is what an eager step gives for it -- both checked against the float64 formulas."""
    torch.manual_seed(3)
    est = fewbit.variance.VarianceEstimator(fewbit.RandomizedLinear(N_IN, N_OUT, proj_dim_ratio=0.25, matmul='rademacher', device=DEV, dtype=dtype))
    x = torch.zeros(B, N_IN, device=DEV, dtype=dtype)
    w = torch.zeros(B, N_OUT, device=DEV, dtype=dtype)
    fills = [tuple(t.to(dtype) for t in _operands('randn', dtype, 500 + i)) for i in range(2)]
    x.copy_(fills[0][0])
    w.copy_(fills[0][1])

    def step():
        return torch.autograd.grad(est(x), [est.model.weight], w)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    steps = est.state.step
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    assert est.state.step == steps + 1
    held = est.variance                                              # outputs of the graph: rewritten by every replay
    seen = []
    for fx, fw in fills:
        x.copy_(fx)
        w.copy_(fw)
        g.replay()
        torch.cuda.synchronize()
        assert est.variance is held
        _check_triple(held, fx, fw, B, B // 4, False, f'captured {NAME(dtype)}')
        seen.append([v.clone() for v in held])
    assert all(not torch.equal(a, b) for a, b in zip(*seen))
    for fx, fw in fills:                                             # eager steps on the same fills meet the same bound: the two agree
        x.copy_(fx)
        w.copy_(fw)
        step()
        torch.cuda.synchronize()
        assert est.variance is not held
        _check_triple(est.variance, fx, fw, B, B // 4, False, f'eager {NAME(dtype)}')
