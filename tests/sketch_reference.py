"""Host model of the random matrix S behind fewbit_hip_sketch (fewbit_amd/csrc/fewbit_sketch.hip): the same formulas,
evaluated with numpy -- a pure function of (seed, row, column).  Test infrastructure (the checker), never the product path.

    philox4x32(c0..c3, k0, k1)      Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
                                    SC'11), vectorised over arrays of counters
    rademacher(seed, rows, cols)    +-1 matrix S[rows x cols]
    xoshiro128pp(state)             xoshiro128++ 1.0 (Blackman & Vigna 2019, reference xoshiro128plusplus.c), vectorised
    gaussian(seed, rows, cols, dt)  N(0,1) by Box-Muller on 16-bit uniforms, rounded to the operand dtype `dt`; the 32-bit words
                                    come from two xoshiro128++ streams per (row, 256-column block, octet parity), each seeded
                                    by one Philox call
"""
import numpy as np
import torch

M32 = np.uint64(0xffffffff)


def philox4x32(c0, c1, c2, c3, k0, k1, rounds=10):
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = np.uint64(k0 & 0xffffffff), np.uint64(k1 & 0xffffffff)
    for _ in range(rounds):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & M32, p0 & M32, n0, n2
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def _key(seed):
    seed &= 0xffffffffffffffff
    return seed & 0xffffffff, seed >> 32


def rademacher(seed: int, nrows: int, ncols: int, row0: int = 0, col0: int = 0) -> torch.Tensor:
    i = (row0 + np.arange(nrows, dtype=np.uint64))[:, None]
    r = (col0 + np.arange(ncols, dtype=np.uint64))[None, :]
    s, h, j = (r % 256) // 16, (r // 8) % 2, r % 8
    words = philox4x32(i, 2 * (r // 256) + h, 0, 0, *_key(seed))
    word = np.choose((s // 4).astype(np.int64) + np.zeros(i.shape, dtype=np.int64), words)
    bit = (word >> (np.where(j % 2 == 1, 31, 15).astype(np.uint64) - (np.uint64(4) * (s % 4) + j // 2))) & np.uint64(1)
    return torch.from_numpy(np.where(bit == 1, -1.0, 1.0).astype(np.float32))


def xoshiro128pp(state):
    """one step for arrays of states (a list of four uint64 arrays holding 32-bit values): returns (output, new state)"""
    s0, s1, s2, s3 = state

    def rotl(x, k):
        return ((x << np.uint64(k)) | (x >> np.uint64(32 - k))) & M32

    result = (rotl((s0 + s3) & M32, 7) + s0) & M32
    t = (s1 << np.uint64(9)) & M32
    s2 = s2 ^ s0
    s3 = s3 ^ s1
    s1 = s1 ^ s2
    s0 = s0 ^ s3
    s2 = s2 ^ t
    s3 = rotl(s3, 11)
    return result, [s0, s1, s2, s3]


def gaussian_words(seed: int, i, r):
    """the 32-bit word behind S[i][r] (arrays, broadcast against each other): with b = r // 256, s = (r % 256) // 16,
    h = (r // 8) % 2, q = (r % 8) // 2: output number 2 s + q % 2 of the xoshiro128++ stream whose state is
    philox(i, 2 b + h, q // 2, 2) -- stream q // 2 feeds operand dwords 2 (q // 2) and 2 (q // 2) + 1 of every MFMA step of the block"""
    i, r = np.broadcast_arrays(np.asarray(i, dtype=np.uint64), np.asarray(r, dtype=np.uint64))
    s, h, q = (r % 256) // 16, (r // 8) % 2, (r % 8) // 2
    state = list(philox4x32(i, 2 * (r // 256) + h, q // 2, 2, *_key(seed)))
    n = (2 * s + q % 2).astype(np.int64)
    word = np.zeros(i.shape, dtype=np.uint64)
    for k in range(int(n.max()) + 1 if n.size else 0):
        out, state = xoshiro128pp(state)
        word = np.where(n == k, out, word)
    return word


def gaussian(seed: int, nrows: int, ncols: int, dtype: torch.dtype = torch.bfloat16, row0: int = 0, col0: int = 0,
             rounded: bool = True) -> torch.Tensor:
    i = (row0 + np.arange(nrows, dtype=np.uint64))[:, None]
    r = (col0 + np.arange(ncols, dtype=np.uint64))[None, :]
    j = r % 8
    w = gaussian_words(seed, i, r)
    u1 = ((w & np.uint64(0xffff)).astype(np.float64) + 0.5) / 65536.0
    u2 = (w >> np.uint64(16)).astype(np.float64) / 65536.0
    rad = np.sqrt(-2.0 * np.log(u1))
    z = np.where(j % 2 == 0, rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2))
    t = torch.from_numpy(z)
    if not rounded:
        return t
    op = torch.float16 if dtype == torch.float16 else torch.bfloat16        # fp32 inputs run on the bf16 pipe
    return t.to(torch.float32).to(op).to(torch.float32)


def matrix(dist: str, seed: int, nrows: int, ncols: int, dtype: torch.dtype = torch.bfloat16, row0: int = 0, col0: int = 0):
    if dist == 'rademacher':
        return rademacher(seed, nrows, ncols, row0, col0)
    return gaussian(seed, nrows, ncols, dtype, row0, col0)


# ---- one-term sums: the exact tests of the product kernels (tests/test_gpu_sketch_exact.py, tests/test_sketch_exact_host.py) ----------
# If every column of M has exactly ONE nonzero entry, every output is a sum of one product and zeros: bit-exact whatever the stage order,
# the slicing or the association of the fp32 sums -- the result names the row, the column, the sign and every rounding.
ONE_TERM_STEP = 277             # prime, and coprime to both row counts below: f -> 277 f mod rows visits every row
ONE_TERM_ROWS = 645             # 2 * 256 + 128 + 5: a last stage with 5 valid rows (most of its octets lie wholly outside)
ONE_TERM_ROWS_SLICED = 3717     # 3072 + 645: the library cuts rows into slices of at least 1024 (645 rows are one slice whatever is asked for);
#                                 three slices of 1280 rows, the last one 4 * 256 + 128 + 5 rows long
ONE_TERM_FEATURES = (264, 261, 520)     # a second column tile of one chunk; the ragged path; 512 + one chunk (the 128 x 512 tile)
ONE_TERM_PROJ = (130, 257)
ONE_TERM_SCALES = (1.0, -0.5, None)     # None: 1 / proj


def one_term_phases(rows: int, features: int) -> int:
    """calls after which every row of M has been the nonzero row of some column (at least three: one per scale)"""
    return max(3, -(-rows // features))


def one_term_rows(rows: int, features: int, phase: int) -> np.ndarray:
    """the nonzero row of every column in call number `phase`: column f -> 277 (f + features * phase) mod rows"""
    return (ONE_TERM_STEP * (np.arange(features, dtype=np.int64) + features * phase)) % rows


def one_term_values(features: int, dtype: torch.dtype, seed: int) -> torch.Tensor:
    """randn scaled by a power of two per column, 2^-20 ... 2^20 (fp16: 2^-6 ... 2^6), in `dtype`"""
    g = torch.Generator().manual_seed(seed)
    span = 6 if dtype == torch.float16 else 20
    e = torch.randint(-span, span + 1, (features, ), generator=g)
    return (torch.randn(features, generator=g) * torch.exp2(e.float())).to(dtype)


def operand(m: torch.Tensor) -> torch.Tensor:
    """M as the matrix pipe gets it, in float32: fp32 rounded to bf16 (to nearest even), 16-bit input as it is"""
    op = torch.float16 if m.dtype == torch.float16 else torch.bfloat16
    return m.to(op).to(torch.float32)


def one_term_expected(S: torch.Tensor, r, values: torch.Tensor, scale: float, bf16_partials: bool = False) -> torch.Tensor:
    """out[i, f] of a call whose column f holds values[f] at row r[f] and zeros elsewhere, in float32 arithmetic throughout:
    S[i, r] * op(m), rounded to bf16 when the slices exchange bf16 partial sums, times float32(scale), one rounding to the dtype of M"""
    S = S.to(torch.float32).cpu()
    v = S[:, torch.as_tensor(r, dtype=torch.int64)] * operand(values.cpu())[None, :]
    if bf16_partials:
        v = v.to(torch.bfloat16).to(torch.float32)
    return (v * torch.tensor(scale, dtype=torch.float32)).to(values.dtype)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def exact_mismatches(got: torch.Tensor, want: torch.Tensor, allowance=None) -> torch.Tensor:
    """mask of the entries that differ: bit for bit, except that NaN matches NaN (payloads are not compared) and zeros are compared by
    value; `allowance` (broadcastable, absolute, 0 where nothing is allowed) is for Gaussian products among the fp32 subnormals"""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    ok = (_bits(got) == _bits(want)) | (torch.isnan(got) & torch.isnan(want)) | ((got == 0) & (want == 0))
    if allowance is not None:
        ok |= (allowance > 0) & ((got.double() - want.double()).abs() <= allowance)
    return ~ok


def subnormal_allowance(values: torch.Tensor, scale: float) -> torch.Tensor:
    """Gaussian S only: |m| < 2^-100 puts s * m among the fp32 subnormals, where it need not be exact -- 2^-149 |scale| there, 0 elsewhere"""
    tiny = operand(values.cpu()).abs() < 2.0**-100
    return torch.where(tiny, torch.tensor(2.0**-149 * abs(scale), dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64))[None, :]


# The settings of the one-term sweep: `tune` values (keys of cabi.tune_sketch_*; a key not named is -1, the policy), the distributions
# and dtypes they are run with.  sketch_convert only acts on fp32 input, sketch_materialise only on the Gaussian sketch.
# tests/test_sketch_exact_host.py checks that, per distribution and dtype, every kernel variant appears in the plans of this list.
_ALL = ('rademacher', 'gaussian')
_F32, _F16, _BF16 = torch.float32, torch.float16, torch.bfloat16
EXACT_SETTINGS = (
    (dict(waves=4, halves=1, materialise=0), _ALL, (_F32, _F16, _BF16)),                                   # fused, 128 x 256 tile
    (dict(waves=8, halves=1, materialise=0), _ALL, (_F32, _F16, _BF16)),                                   # fused, 256 x 256 tile
    (dict(halves=2, materialise=0), _ALL, (_F32, _F16, _BF16)),                                            # 128 x 512 tile
    (dict(waves=4, halves=1, materialise=1), ('gaussian', ), (_F16, _BF16)),                               # S from memory
    (dict(waves=8, halves=1, slices=3, partials=0, materialise=0), _ALL, (_F32, _F16, _BF16)),             # sliced, fp32 partial sums
    (dict(waves=4, halves=1, slices=3, partials=1, materialise=0), _ALL, (_F16, _BF16)),                   # sliced, bf16 partial sums (bf16)
    (dict(halves=2, slices=3, partials=1, materialise=0), _ALL, (_F16, _BF16)),                            # the same on the 128 x 512 tile
    (dict(waves=8, halves=1, slices=3, partials=1, materialise=1), ('gaussian', ), (_F16, _BF16)),         # S from memory, sliced
    (dict(waves=4, halves=1, convert=1, materialise=0), _ALL, (_F32, )),                                   # fp32 rounded to bf16 first
    (dict(waves=8, halves=1, convert=1, materialise=1), ('gaussian', ), (_F32, )),                         # ... S from memory
    (dict(halves=2, convert=1, slices=3, partials=1, materialise=0), _ALL, (_F32, )),                      # ... 128 x 512, bf16 partial sums
    (dict(waves=8, halves=1, convert=1, slices=3, partials=0, materialise=0), _ALL, (_F32, )),             # ... fp32 partial sums
    (dict(waves=4, halves=1, convert=1, slices=3, partials=1, materialise=1), ('gaussian', ), (_F32, )),   # ... S from memory, bf16 partial sums
    (dict(waves=4, halves=1, convert=0, slices=3, materialise=0), _ALL, (_F32, )),                         # fp32 staged in the kernel, sliced
)
TUNE_KEYS = ('slices', 'waves', 'halves', 'convert', 'partials', 'materialise')


def exact_cases():
    """(distribution, dtype, tune dict) of every case of the sweep"""
    return [(dist, dtype, tune) for tune, dists, dtypes in EXACT_SETTINGS for dist in dists for dtype in dtypes]


def expected_plan(dist: str, dtype: torch.dtype, tune: dict, rows: int) -> dict:
    """what a setting of EXACT_SETTINGS asks for (every feature count of the sweep is wider than one column tile): the fields the GPU
    test asserts on describe_sketch before it trusts a case to have run the kernel variant it is named after"""
    converted = dtype == torch.float32 and tune.get('convert', -1) == 1
    operand_bf16 = dtype == torch.bfloat16 or converted
    gz = 3 if tune.get('slices', -1) == 3 and rows >= 3072 else 1
    if gz == 1:
        partial = 'fp32' if converted else None
    else:
        partial = 'bf16' if operand_bf16 and tune.get('partials', -1) == 1 and dtype != torch.float16 else 'fp32'
    return {'wide': tune.get('halves', -1) == 2,
            'tile': '128x512' if tune.get('halves', -1) == 2 else '128x256' if tune['waves'] == 4 else '256x256',
            'from_memory': dist == 'gaussian' and tune.get('materialise', -1) == 1 and (dtype != torch.float32 or converted),
            'converted': converted, 'gz': gz, 'partial_sums': partial}
