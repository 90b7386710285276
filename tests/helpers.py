"""Shared helpers for the parity tests (bit-exact views, fixture decoding, ULP distance, captured steps of the sampled transforms, the
per-column error measure of the sampled transforms and their structured inputs)."""
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / 'tests' / 'golden'
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}


def from_raw(a: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    """Inverse of gen_golden.raw(): uint16 words -> bf16/fp16 tensor, float32 stays."""
    if dtype in (torch.bfloat16, torch.float16):
        return torch.from_numpy(a.astype(np.uint16).view(np.int16).copy()).view(dtype)
    return torch.from_numpy(a.astype(np.float32).copy())


def bits(t: torch.Tensor) -> torch.Tensor:
    """Integer view for bit-exact comparison."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.view(torch.int16)
    return t


def assert_bit_equal(a: torch.Tensor, b: torch.Tensor, what: str = '', nan_equal: bool = True):
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    ia, ib = bits(a), bits(b)
    neq = ia != ib
    if nan_equal and a.is_floating_point():
        neq &= ~(torch.isnan(a) & torch.isnan(b))        # NaN payload/sign is not part of parity
    if neq.any():
        idx = neq.flatten().nonzero().flatten()[:8]
        raise AssertionError(f'{what}: {int(neq.sum())} of {a.numel()} differ, first at {idx.tolist()}: '
                             f'{a.flatten()[idx].tolist()} vs {b.flatten()[idx].tolist()}')


def ordered(t: torch.Tensor) -> torch.Tensor:
    """Map floats to integers so that adjacent representable values differ by 1."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        i = t.view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    i = t.view(torch.int16).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7fff), i)


def ulp_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """|a-b| in units of representable steps of the common dtype (NaN==NaN -> 0)."""
    d = (ordered(a) - ordered(b)).abs()
    both_nan = torch.isnan(a.detach().cpu()) & torch.isnan(b.detach().cpu())
    return torch.where(both_nan, torch.zeros_like(d), d)


def load_tables() -> dict:
    """The built-in quantization tables as float64 numpy arrays (the product's own data file)."""
    with np.load(ROOT / 'fewbit_amd' / 'data' / 'builtin.npz') as z:
        return {k: z[k].copy() for k in z.files}


def forward_value_ok(x: torch.Tensor, y: torch.Tensor, y_ref: torch.Tensor, tight: bool = False) -> torch.Tensor:
    """Element-wise verdict for forward activation values (the only floating-point parity in the path).

    The reference's forward values are ATen's (third-party: MKL vsCdfNorm for contiguous fp32, Sleef erf for
    16-bit and strided inputs -- the two already disagree with each other by up to 5 fp32 steps for x>0 and by
    the full cancellation noise of 1+erf(x/sqrt2) for x<0).  So the bar is stated on the shared formula
    y = x*0.5*(1+erf(x*sqrt(1/2))) evaluated in fp32:
      loose (vs ATen output):   |dy| <= max(1 step of the output dtype at y_ref, 2^-21 * |x|)
      tight (vs the formula with a correctly rounded erf): |dy| <= max(1 step, 2^-24 * |x|)
    2^-24*|x| is what ONE fp32 rounding step of erf costs after the *0.5x scaling.  Non-finite x are excluded
    (ATen itself returns NaN for +inf on some paths); NaN must map to NaN.
    """
    xf, yf, rf = x.detach().cpu().double(), y.detach().cpu().double(), y_ref.detach().cpu().double()
    step_ok = ulp_distance(y, y_ref) <= 1
    scale = 2.0**-24 if tight else 2.0**-21
    abs_ok = (yf - rf).abs() <= scale * xf.abs()
    nan_ok = torch.isnan(xf) & torch.isnan(yf)
    skip = torch.isinf(xf)
    return step_ok | abs_ok | nan_ok | skip


# Input data of the reference's CUDA smoke test (fewbit/cuda/codec_test.cu: TestCodecBlock :62-64, TestGelu :93-98).
# The reference only prints the results; the two vectors pin each other: with the built-in 3-bit GELU table the 16
# inputs fall into exactly the 16 codes of the codec smoke test.
REF_SMOKE_CODES = (6, 5, 6, 1, 7, 0, 4, 2, 2, 3, 0, 4, 5, 5, 6, 7)
REF_SMOKE_GELU_INPUTS = (2.29811567e+00, 6.10855860e-01, 2.29811567e+00, -8.11248159e-01, 9.99900000e+02, -2.49798704e+00,
                         2.26182064e-01, -4.26290283e-01, -4.26290283e-01, -1.00155338e-01, -2.49798704e+00, 2.26182064e-01,
                         6.10855860e-01, 6.10855860e-01, 2.29811567e+00, 9.99900000e+02)


# ---- full-size inputs of the BASELINE configs (shared by tests/golden/gen_golden.py, which runs the REFERENCE on them and
# commits SHA-256 digests, and by tests/test_gpu_parity.py, which regenerates them on the GPU box) -------------------------
FULL_SIZE_CASES = {
    # name: (function, bits, dtype key, rows, cols)
    'c2_gelu3_bf16_4096x4096': ('gelu', 3, 'bf16', 4096, 4096),
    'c3_silu2_f16_8192x8192': ('silu', 2, 'f16', 8192, 8192),
    'c3_silu4_f16_8192x8192': ('silu', 4, 'f16', 8192, 8192),
    'c4shard_gelu3_bf16_8192x4096': ('gelu', 3, 'bf16', 8192, 4096),
}


def border_specials(inner_borders: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """NaN (both signs), +-inf, +-0, every border and its two neighbours in `dtype`, +-100, +-200."""
    b = inner_borders.to(dtype)
    it = torch.int32 if dtype == torch.float32 else torch.int16
    nb = b.view(it)
    fixed = torch.tensor([float('nan'), float('inf'), -float('inf'), 0.0, -0.0, 100.0, -100.0, 200.0, -200.0, 1e-30, -1e-30]).to(dtype)
    neg_nan = torch.tensor([-1], dtype=it).view(dtype)
    return torch.cat([fixed, b, (nb + 1).view(dtype), (nb - 1).view(dtype), neg_nan])


def full_size_inputs(case: str, tables: dict):
    """(x, gy, inner borders, levels) of a BASELINE-size case: seeded host randn cast to the dtype, with the
    special values spliced in at the start and at the end of x."""
    name, bits, dt, rows, cols = FULL_SIZE_CASES[case]
    dtype = DTYPES[dt]
    borders = torch.tensor(tables[f'{name}{bits:02d}-borders']).to(dtype)[1:-1].contiguous()
    levels = torch.tensor(tables[f'{name}{bits:02d}-levels']).to(dtype)
    x = torch.randn(rows * cols, generator=torch.Generator().manual_seed(0)).to(dtype)
    gy = torch.randn(rows * cols, generator=torch.Generator().manual_seed(1)).to(dtype)
    sp = border_specials(borders, dtype)
    x[:sp.numel()] = sp
    x[-sp.numel():] = sp
    return x, gy, borders, levels


# ---- BASELINE config 4 in full: 4 tensors of 16384x4096 bf16, each cut in two halves -> 8 shards, tensor t half h on GPU 2t+h
# (SURVEY 8(e)).  The reference runs on each WHOLE tensor (tests/golden/gen_golden.py c4); a shard's expected state / gx is the
# slice of that run at the shard's offsets, which is exactly the claim "sharding == slicing the unsharded result".
C4_TENSORS, C4_ROWS, C4_COLS, C4_BITS = 4, 16384, 4096, 3


def c4_tensor_inputs(t: int, tables: dict):
    """(x, gy, inner borders, levels) of whole tensor `t` of config 4: seeded host randn, the special values spliced in at
    both ends AND on both sides of the cut between its two shards."""
    dtype = torch.bfloat16
    borders = torch.tensor(tables['gelu03-borders']).to(dtype)[1:-1].contiguous()
    levels = torch.tensor(tables['gelu03-levels']).to(dtype)
    n = C4_ROWS * C4_COLS
    x = torch.randn(n, generator=torch.Generator().manual_seed(400 + t)).to(dtype)
    gy = torch.randn(n, generator=torch.Generator().manual_seed(500 + t)).to(dtype)
    sp = border_specials(borders, dtype)
    x[:sp.numel()] = sp
    x[-sp.numel():] = sp
    x[n // 2 - sp.numel():n // 2] = sp
    x[n // 2:n // 2 + sp.numel()] = sp
    return x, gy, borders, levels


def c4_shard(rank: int):
    """(tensor index, element range, state byte range) of GPU `rank`'s shard of config 4"""
    # (sharding.py loaded by path, not through the package: tests/golden/gen_golden.py calls this with the REFERENCE's
    # operator library loaded, which registers the same torch.ops namespace as the package's own)
    import importlib.util
    spec = importlib.util.spec_from_file_location('_fewbit_sharding', ROOT / 'fewbit_amd' / 'sharding.py')
    sharding = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sharding)
    shard_range, state_range = sharding.shard_range, sharding.state_range
    t, h = divmod(rank, 2)
    begin, end = shard_range(C4_ROWS * C4_COLS, 2, h)
    return t, (begin, end), state_range(begin, end, C4_BITS)


def sha256_of(t: torch.Tensor) -> str:
    import hashlib
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


# ---- the layer's sampled transforms ('dct', 'dft') inside a hipGraph (tests/test_gpu_dct.py, tests/test_gpu_dft.py) -------------------
BASE = 0x7654321                     # the host draw the recorded seed kernel starts from (linear._draw_seed pinned to it)


def captured_step_replays_fresh_rows(kind, rows, features, p, dtype, warm_rows, dev='cuda:0'):
    """warm up the layer (matmul=kind) eagerly at `warm_rows`, capture one fwd + bwd step at `rows`, replay it three times; every replay must
    equal the explicit product on the rows of its seed, and replays must differ.  The caller pins linear._draw_seed to BASE."""
    import fewbit
    from fewbit_amd import cabi, cabi_x, linear
    lin = fewbit.RandomizedLinear(features, 32, proj_dim=p, matmul=kind, bias=False, device=dev, dtype=dtype)
    x = torch.randn(rows, features, device=dev, dtype=dtype, requires_grad=True)
    wgt = torch.randn(rows, 32, device=dev, dtype=dtype)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xw = torch.randn(warm_rows, features, device=dev, dtype=dtype, requires_grad=True)
        torch.autograd.grad((lin(xw) * torch.randn(warm_rows, 32, device=dev, dtype=dtype)).sum(), lin.weight)
    torch.cuda.current_stream().wait_stream(side)
    counter = linear._replay_counter(torch.device(dev))
    c0 = int(counter)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gw, = torch.autograd.grad((lin(x) * wgt).sum(), lin.weight)
    seen = []
    for r in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert int(counter) == c0 + r + 1
        idx = cabi.sampled_rows(cabi.mix_sketch_seed(BASE, c0 + r), rows, p).to(dev)
        if kind == 'dct':
            want = cabi.sampled_dct(wgt, idx).T @ cabi.sampled_dct(x.detach(), idx, rows / p)
        else:
            gr, gi = cabi_x.sampled_dft(wgt, idx)
            xr, xi = cabi_x.sampled_dft(x.detach(), idx, rows / p)
            want = gr.T @ xr + gi.T @ xi
        assert torch.allclose(gw, want, rtol=1e-4, atol=1e-3), (r, float((gw - want).abs().max()))
        seen.append(gw.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ---- the sampled transforms per feature column (tests/test_gpu_transform_columns.py, tests/test_transform_error_model.py) ----------------
# Both kernel pairs transform the features (2c, 2c + 1) as ONE complex column, so the error of column c scales with the RMS of the pair
# (c, c ^ 1).  The error of an entry is measured against the RMS of its own input column (= the RMS of its output column: the transforms are
# orthonormal); the pair measure divides by the larger RMS of the two columns of its pair.
U_F32 = 2.0**-24
ERROR_FACTOR = 4.0                   # bound = 4 x max(E_ref, u log2 N): a correct packed four-step stays within 1.3 x the fp32 reference
TRANSFORM_FAMILIES = ('white noise', 'mean 1000 sigma', 'random walk', 'single spike', 'pure tone', 'alternating', 'scales per pair')


def column_rms(x: torch.Tensor) -> torch.Tensor:
    """RMS of every column of a (rows, features) matrix, float64"""
    return x.double().pow(2).mean(0).sqrt()


def pair_rms(x: torch.Tensor) -> torch.Tensor:
    """per column c: the larger RMS of the columns c and c ^ 1 (a last column without a partner: its own)"""
    r = column_rms(x)
    mate = torch.arange(r.numel(), device=r.device) ^ 1
    mate = torch.where(mate < r.numel(), mate, torch.arange(r.numel(), device=r.device))
    return torch.maximum(r, r[mate])


def _planes(t: torch.Tensor) -> torch.Tensor:
    """a complex (p, features) result as the kernel's (2, p, features) planes; a real one as it is; float64"""
    return torch.stack([t.real, t.imag]).double() if t.is_complex() else t.double()


def normalised_error(got: torch.Tensor, want: torch.Tensor, x: torch.Tensor, pair: bool = False) -> torch.Tensor:
    """|got - want| / RMS of the input column of each entry (pair: / the larger RMS of the columns 2c, 2c + 1).  `got`, `want`: sampled
    rows (p, features) or planes (2, p, features), complex allowed; `x`: the input (rows, features), already rounded to the kernel's dtype.
    An entry of an all-zero column (pair) counts 0 when exact, inf otherwise."""
    got, want = _planes(got), _planes(want).to(got.device)
    rms = (pair_rms(x) if pair else column_rms(x)).to(got.device)
    err = (got - want).abs()
    return torch.where(rms > 0, err / torch.where(rms > 0, rms, torch.ones_like(rms)), torch.where(err == 0, 0.0, float('inf')))


def reference_error(ref32: torch.Tensor, want: torch.Tensor, x: torch.Tensor, pair: bool = False) -> float:
    """E_ref: the largest normalised error of the fp32 reference on the same data (over the same sampled rows)"""
    return float(normalised_error(ref32, want, x, pair).max())


def transform_error_check(got, want, x, e_ref: float, rel: float, pair: bool = False, floor: float = 0.0):
    """The per-entry criterion of the sampled transforms:

        |err| <= rel |want| + 4 max(E_ref, u log2 N) RMS_c + floor

    rel: one rounding of the fp32 result to the output dtype (0 for fp32 results); floor: 2^-24 for fp16 results (subnormal steps);
    RMS_c: the column's (pair: the pair's).  -> (ok, worst |err| / bound, kernel-to-reference ratio = the largest normalised error left
    after the output rounding, / max(E_ref, u log2 N): the criterion is this ratio <= 4, with every entry finite)"""
    rows = x.shape[0]
    unit = max(e_ref, U_F32 * math.log2(rows))
    got, want = _planes(got), _planes(want).to(got.device)
    rms = (pair_rms(x) if pair else column_rms(x)).to(got.device)
    err = (got - want).abs()
    tol = rel * want.abs() + ERROR_FACTOR * unit * rms + floor
    ok = bool((err <= tol).all()) and bool(torch.isfinite(got).all())
    left = (err - rel * want.abs() - floor).clamp_min(0.0)
    excess = torch.where(rms > 0, left / torch.where(rms > 0, rms, torch.ones_like(rms)), torch.where(left == 0, 0.0, float('inf')))
    return ok, float((err / tol.clamp_min(1e-300)).max()), float(excess.max()) / unit


def transform_input(family: str, kind: str, rows: int, features: int, dtype: torch.dtype, seed: int):
    """(x, k0): a host (rows, features) matrix of `family` (TRANSFORM_FAMILIES, or 'partners': columns 2c and 2c + 1 2^20 apart -- 2^6 for
    fp16 --, the larger one alternating between the two, and the pair (2, 3) all zero), rounded to `dtype` and returned as float64; k0:
    the bin of the pure tone (of the DCT-II basis for kind 'dct', of the DFT for 'dft').  Amplitudes and scales differ between pairs and
    are equal within one: the coupling inside a pair is the 'partners' family's.  Every exact output stays finite in `dtype`:
    the fp16 mean is 100 sigma (1000 sigma x sqrt(2^18) is beyond fp16), the walk is divided by sqrt(rows)."""
    g = torch.Generator().manual_seed(seed)
    n = torch.arange(rows, dtype=torch.float64)[:, None]
    col = torch.arange(features)
    amp = (1.0 + (col // 2) % 5).double()                                  # equal within a pair (unequal pairs: 'partners')
    k0 = rows // 3 + 7
    fp16 = dtype == torch.float16
    if family == 'white noise':
        x = torch.randn(rows, features, generator=g, dtype=torch.float64)
    elif family == 'mean 1000 sigma':
        x = torch.randn(rows, features, generator=g, dtype=torch.float64) + (100.0 if fp16 else 1000.0)
    elif family == 'random walk':
        x = torch.randn(rows, features, generator=g, dtype=torch.float64).cumsum(0) / math.sqrt(rows)
    elif family == 'single spike':
        x = torch.zeros(rows, features, dtype=torch.float64)
        x[torch.randint(0, rows, (features, ), generator=g), col] = amp
    elif family == 'pure tone':
        if kind == 'dct':
            x = torch.cos(math.pi * (2 * n + 1) * k0 / (2 * rows)) * amp
        else:
            phase = torch.rand(features, generator=g, dtype=torch.float64) * 2 * math.pi
            x = torch.cos(2 * math.pi * ((n * k0) % rows) / rows + phase) * amp
    elif family == 'alternating':
        x = (1.0 - 2.0 * (n % 2)) * amp
    elif family == 'scales per pair':
        s = torch.tensor((2.0**-6, 1.0, 2.0**6) if fp16 else (2.0**-30, 1.0, 2.0**30), dtype=torch.float64)
        x = torch.randn(rows, features, generator=g, dtype=torch.float64) * s[(col // 2) % 3]
    elif family == 'partners':
        big = 2.0**6 if fp16 else 2.0**20
        s = torch.where((col % 2) == ((col // 2) % 2), big, 1.0).double()
        x = torch.randn(rows, features, generator=g, dtype=torch.float64) * s
        x[:, 2:4] = 0.0
    else:
        raise ValueError(family)
    return x.to(dtype).double(), k0


def transform_rows(rows: int, k0: int, draws: int, seed: int) -> torch.Tensor:
    """the sampled rows of a structured case: the corners 0, N/2, N-1, the tone's bins k0, N-k0, and `draws` random rows (host int64)"""
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.tensor([0, rows // 2, rows - 1, k0, rows - k0]), torch.randint(0, rows, (draws, ), generator=g)])


# ---- the sampled transforms against their float64 rows (tests/test_gpu_transform_splits.py; shown to have teeth in tests/test_transform_rows_host.py) ----
TRANSFORM_EPS = 3e-6                 # the fp32 four-step FFT stays within 3e-6 max|y| of the float64 transform
ROUNDING = {torch.float32: 0.0, torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8}      # one rounding of the fp32 result to the result's dtype


def sampled_rows_check(got, want, rel: float = 0.0):
    """The criterion every sampled-transform test states, per entry:

        |got - want| <= rel |want| + 3e-6 max|want|

    `got`: the kernel's (p, features) rows, or the (2, p, features) planes of the DFT (any float dtype, host or device); `want`: the
    float64 rows of the same shape (numpy or torch), complex (p, features) for the planes; `rel`: ROUNDING of the result's dtype.
    -> (ok, the worst |err| / bound).  A result of another shape or with a non-finite entry is not ok."""
    want = torch.as_tensor(np.asarray(want))
    want = torch.stack([want.real, want.imag]).double() if want.is_complex() else want.double()
    got = got.detach().cpu().double()
    if got.shape != want.shape:
        return False, float('inf')
    if not bool(torch.isfinite(got).all()):
        return False, float('inf')
    err = (got - want).abs()
    tol = rel * want.abs() + TRANSFORM_EPS * float(want.abs().max())
    return bool((err <= tol).all()), float((err / tol.clamp_min(1e-300)).max())


CAPTURE_CHILD = '''
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
from fewbit_amd import linear
import helpers
torch.manual_seed(0)
linear._draw_seed = lambda generator: helpers.BASE
helpers.captured_step_replays_fresh_rows({kind!r}, 32768, 64, 3276, torch.float32, 512)
print('captured 32768-row step ok')
'''


def large_tile_capture_in_a_fresh_process(kind):
    """32768 rows (LDS tiles above 64 KiB) captured in a fresh process whose only eager call was at 512 rows"""
    code = CAPTURE_CHILD.format(root=str(ROOT), tests=str(ROOT / 'tests'), kind=kind)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'captured 32768-row step ok' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- the same input through a kernel's tile body and through its element-wise tail (tests/test_gpu_tail_body.py, tests/test_gpu_step1_exhaustive.py) ----
# A streaming activation kernel computes an element in a whole tile (64 x U groups, vectorised) or, where the tensor does not fill one, in the
# element-wise tail of the last wave: separate code, separate conversions.  BODY_N = 65 x 1024 elements has no tail at U = 1 and at U = 2, and the wide
# backward (one group of slack) still covers its first BODY_COVERED elements with tiles; a call of at most TAIL_N = 511 elements (63 full groups and
# a ragged one of 7) has no tile at all.
BODY_N, BODY_COVERED, TAIL_N = 66560, 66048, 511
STREAM_TUNE_KEYS = ('waves_per_cu', 'chunk', 'lut_chunk', 'lut_blocks_per_cu', 'lut_min', 'u_fwd', 'u_bwd', 'u_step1')


# the parameter sets of the 1-bit family: values the 16-bit dtypes hold exactly and values they do not (0.3, 1/3, 0.01, 0.1)
STEP1_CASES = [('hardshrink', (0.5, )), ('hardshrink', (0.3, )), ('hardshrink', (1 / 3, )), ('hardsigmoid', ()), ('hardtanh', (-1.0, 1.0)),
               ('hardtanh', (-0.3, 0.7)), ('leaky_relu', (0.01, )), ('leaky_relu', (0.1, )), ('leaky_relu', (0.3, )), ('leaky_relu', (0.5, )), ('relu', ()),
               ('relu6', ()), ('softshrink', (0.5, )), ('softshrink', (0.3, )), ('softshrink', (1 / 3, )), ('threshold', (1.0, 3.0)), ('threshold', (0.3, -0.1))]
GEOMETRIES = (('body', 1), ('body', 2), ('tail', 1), ('tail', 2))          # (where every element is computed, groups per lane per stage)


def case_id(v) -> str:
    """pytest id of a function name or of its parameter tuple"""
    return v if isinstance(v, str) else '-'.join(f'{q:.3g}' for q in v)


def kinks(p) -> tuple:
    """0, +-p0, p1, +-3 and 6: the kink values of the 1-bit family, whose fp32 neighbours every fp32 probe includes"""
    p0, p1 = (tuple(p) + (0.0, 0.0))[:2]
    return (0.0, p0, -p0, p1, 3.0, -3.0, 6.0)


def set_groups_per_lane(u: int) -> None:
    """force U of every streaming kernel that is built with more than one (fewbit_hip_tune)"""
    from fewbit_amd import cabi
    cabi.tune(u_fwd=u, u_bwd=u, u_step1=u)


def run_geometry(where: str, op, *inputs):
    return (run_body if where == 'body' else run_tail)(op, *inputs)


def all_16bit(dtype: torch.dtype) -> torch.Tensor:
    """every pattern of a 16-bit dtype, 0x8000 .. 0xffff then 0x0000 .. 0x7fff"""
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)


def fp32_neighbours(values) -> torch.Tensor:
    """float32(v) and its +-1 and +-2 ulp neighbours, for every v"""
    v = torch.tensor(list(values), dtype=torch.float32).view(torch.int32)
    return torch.cat([v + d for d in (-2, -1, 0, 1, 2)]).view(torch.float32)


def probe_patterns(dtype: torch.dtype, kinks=()) -> torch.Tensor:
    """The inputs of a tail-against-body case: every pattern of a 16-bit dtype; for fp32 the 65 536 patterns k * 65537 mod 2^32 (every exponent, both
    signs), +-0, +-inf, NaN of both signs and the +-1 / +-2 ulp neighbours of every value of `kinks`."""
    if dtype != torch.float32:
        return all_16bit(dtype)
    spread = ((torch.arange(65536, dtype=torch.int64) * 65537) & 0xffffffff).to(torch.int32).view(torch.float32)
    special = torch.tensor([0, -0x80000000, 0x7f800000, -0x00800000, 0x7fc00000, -0x00400000], dtype=torch.int64).to(torch.int32).view(torch.float32)
    x = torch.cat([spread, special, fp32_neighbours(kinks)])
    assert x.numel() <= BODY_COVERED
    return x


def run_body(op, *inputs, dev='cuda:0'):
    """op(*device tensors of BODY_N elements) -> tuple of per-element device tensors, on the inputs extended to BODY_N with their own first elements:
    every input element lies in a whole tile.  -> the outputs of the inputs' own elements, on the host"""
    n = inputs[0].numel()
    assert BODY_N - 1024 <= n <= BODY_COVERED and all(t.numel() == n for t in inputs)
    outs = op(*(torch.cat([t, t[:BODY_N - n]]).to(dev) for t in inputs))
    return tuple(o[:n].cpu() for o in outs)


def run_tail(op, *inputs, dev='cuda:0'):
    """the same through calls of at most TAIL_N elements: every element is computed by the element-wise tail"""
    n = inputs[0].numel()
    on_dev = [t.to(dev) for t in inputs]
    outs = [op(*(d[i:i + TAIL_N] for d in on_dev)) for i in range(0, n, TAIL_N)]
    return tuple(torch.cat(col).cpu() for col in zip(*outs))


def differing(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """positions whose bits differ, two NaNs counting as equal (host tensors of one dtype and shape)"""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    neq = bits(a) != bits(b)
    if a.is_floating_point():
        neq &= ~(torch.isnan(a) & torch.isnan(b))
    return neq
