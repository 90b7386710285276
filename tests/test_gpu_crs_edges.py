"""The column-sampling kernels of LinearCRS (fewbit_amd/csrc/fewbit_crs.hip) at their alignment, size and value edges.  Every reference is
computed on the HOST: the columns from cabi_x.crs_columns(seed, in_features, nopairs), the arithmetic in float64, compared bit for bit
wherever the contract is bit-exact.

  1. every alignment class of the spread kernel: n x (start of out mod 16 bytes) x rows, both directions, three dtypes, cap below, at and above m
  2. the columns the DEVICE evaluates (pos, cols, scale read back through the entry points) at every boundary of the prep kernel
  3. every 16-bit pattern and the fp32 specials through the gather's arithmetic; every bit pattern through the scatter
  4. the layer against float64 in three dtypes, with a derived bound
  5. several randomized layers in one captured step: every layer's backward meets its own forward's seed

The gather's reference, for x of `dtype` and the host's cols / count:

    scale32 = (count.double() * in_features / nopairs).float()
    want    = (x.float().double()[:, cols] * scale32.double()).float().to(dtype)

(the double product of two fp32 numbers is exact, so one rounding to fp32 is the correctly rounded fp32 multiply, subnormal results included;
then the rounding to the dtype).  NaN bits are not part of it: non-NaN results match bit for bit, NaN falls exactly where the reference has
NaN, and a bf16 NaN result is the canonical 0x7fc0 the kernel documents (torch's host conversion writes 0xffff)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi, cabi_x, linear

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
INT = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
ELEMS = {torch.float32: 4, torch.float16: 8, torch.bfloat16: 8}                         # E: elements of one 16-byte piece
U_OUT = {torch.float32: 2.0**-24, torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8}      # one rounding to the dtype
MASK64 = 0xffffffffffffffff


@pytest.fixture(autouse=True)
def native_sketch_on():
    prev = linear.use_native_sketch(True)
    yield
    linear.use_native_sketch(prev)


# ---- the host reference ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_columns(seed, in_features, nopairs):
    """-> (cols int64, count int32, scale32) on the host"""
    cols, count = cabi_x.crs_columns(seed, in_features, nopairs)
    return cols, count, (count.double() * in_features / nopairs).float()


def gather_reference(x, cols, scale32):
    """x: host tensor (rows, in_features) of the kernel's dtype -> (rows, m) of that dtype"""
    return (x.float().double()[:, cols] * scale32.double()).float().to(x.dtype)


def ibits(t):
    return t.contiguous().view(INT[t.dtype])


def assert_gathered(got, want, what):
    """the NaN rule of the module docstring; `got`, `want`: host tensors of one dtype"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), (what, 'NaN in other places', int((torch.isnan(got) != nan).sum()))
    gb, wb = ibits(got), ibits(want)
    bad = (gb != wb) & ~nan
    if bool(bad.any()):
        at = bad.nonzero()[:6].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} differ, first at {at}: '
                             f'{[hex(int(gb[tuple(i)]) & 0xffffffff) for i in at]} vs {[hex(int(wb[tuple(i)]) & 0xffffffff) for i in at]}')
    if got.dtype == torch.bfloat16:
        assert bool((gb[nan] == 0x7fc0).all()), (what, 'a bf16 NaN that is not 0x7fc0')


def assert_bits(got, want, what):
    gb, wb = ibits(got), ibits(want)
    bad = gb != wb
    if bool(bad.any()):
        at = bad.nonzero()[:6].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} differ, first at {at}: '
                             f'{[hex(int(gb[tuple(i)]) & 0xffffffff) for i in at]} vs {[hex(int(wb[tuple(i)]) & 0xffffffff) for i in at]}')


def seed_word(seed):
    """the seed as a device word (int64 holds the same 64 bits)"""
    seed &= MASK64
    return torch.tensor([seed - (1 << 64) if seed >> 63 else seed], dtype=torch.int64, device=DEV)


def coded(rows, cols, dtype, stride):
    """host (rows, cols) tensor whose value tells its position: fp32 r * stride + c + 1 (exact below 2^24); 16-bit: the bit pattern
    0x3800 + (r * stride + c) mod 8192 (finite normals of either format, 2^-15 .. 2^48 as bf16, 0.5 .. 128 as fp16; `stride` odd, so two
    entries of one row, or of one column, never share a value)"""
    code = torch.arange(rows, dtype=torch.int64)[:, None] * stride + torch.arange(cols, dtype=torch.int64)[None, :]
    if dtype == torch.float32:
        assert rows * stride + cols < 2**24
        return (code + 1).float()
    assert stride % 2 == 1 and cols <= 8192 and rows <= 8192
    return (0x3800 + code % 8192).to(torch.int16).view(dtype)


# ---- 1. every alignment class of the spread kernel ------------------------------------------------------------------------------------
def sweep_n(E):
    """the widths of `out`: every residue mod E twice over, and both sides of the first tile boundary along j (2 + ceil(n / E) pieces
    against 64 per tile)"""
    return list(range(1, 2 * E + 2)) + [62 * E - 1, 62 * E, 62 * E + 1, 63 * E, 64 * E + 1]


def sweep_rows(n, E):
    """fewer rows than classes, exactly one group per class, a ragged second group, a third group (P classes, 16 rows per group)"""
    g = 1
    while g < E and n % (2 * g) == 0:
        g *= 2
    P = E // g
    return sorted({r for r in (1, P - 1, P, P + 1, 16 * P, 16 * P + 1, 33 * P + 2) if r > 0})


# gather: (in_features, nopairs, seed) -> m by the host's evaluation; n <= 2E + 1 takes the small shape, the tile-boundary widths the large one
GATHER_SHAPES = {4: ((24, 9, 0x5eed0001, 7), (640, 320, 0x5eed1018, 248)), 8: ((48, 17, 0x5eed0008, 13), (1280, 640, 0x5eed1029, 496))}
SWEEP = [(dtype, n) for dtype in DTYPES for n in sweep_n(ELEMS[dtype])]
SWEEP_IDS = [f'{str(dtype)[6:]}-n{n}' for dtype, n in SWEEP]


def gather_shape(n, E):
    return GATHER_SHAPES[E][0 if n <= 2 * E + 1 else 1]


def scatter_shape(n):
    """scatter: in_features = n, two draws per column (m about 0.86 n, so caps below m exist from n = 2 on)"""
    return n, 2 * n, 0xc0150000 + n


def scatter_caps(n):
    in_features, nopairs, seed = scatter_shape(n)
    m = host_columns(seed, in_features, nopairs)[0].numel()
    return m, sorted({c for c in (1, m - 2, m - 1, m, min(nopairs, in_features)) if c >= 1})


def test_the_sweep_has_caps_below_at_and_above_m():
    for E in (4, 8):
        seen = set()
        for n in sweep_n(E):
            in_features, nopairs, seed, m = gather_shape(n, E)
            assert host_columns(seed, in_features, nopairs)[0].numel() == m and n <= min(nopairs, in_features)
            seen.add('below' if n < m else 'at' if n == m else 'above')
        assert seen == {'below', 'at', 'above'}, (E, seen)
        seen = set()
        for n in sweep_n(E):
            m, caps = scatter_caps(n)
            seen |= {'below' if c < m else 'at' if c == m else 'above' for c in caps}
        assert seen == {'below', 'at', 'above'}, (E, seen)


class Arena:
    """One NaN-filled buffer for all the calls of a case: call i writes a rows x n block that starts `offset` elements past a 16-byte
    boundary, with at least E NaN elements on either side.  The expected image (the NaN around the blocks included) is built on the host and
    compared once."""

    def __init__(self, dtype, calls, n):
        E = ELEMS[dtype]
        self.dtype, self.n, self.blocks, at = dtype, n, [], 0
        for offset, rows in calls:
            at = (at + E + E - 1) // E * E + offset
            self.blocks.append((at, rows, offset))
            at += rows * n + E
        self.size = at + E
        self.want = torch.full((self.size, ), float('nan'), dtype=dtype)
        self.got = torch.full((self.size, ), float('nan'), dtype=dtype, device=DEV)
        assert self.got.data_ptr() % 16 == 0

    def out(self, i):
        at, rows, offset = self.blocks[i]
        view = self.got[at:at + rows * self.n].view(rows, self.n)
        assert view.data_ptr() % 16 == offset * self.got.element_size()
        return view

    def expect(self, i, block):
        at, rows, _ = self.blocks[i]
        assert block.shape == (rows, self.n) and not bool(torch.isnan(block).any())
        self.want[at:at + rows * self.n] = block.reshape(-1)

    def check(self, what):
        torch.cuda.synchronize()
        got = self.got.cpu()
        nan = torch.isnan(self.want)
        ok = torch.equal(torch.isnan(got), nan) and torch.equal(ibits(got)[~nan], ibits(self.want)[~nan])
        if ok:
            return
        for i, (at, rows, offset) in enumerate(self.blocks):                           # which call, and what of it
            lo, hi = at - ELEMS[self.dtype], at + rows * self.n + ELEMS[self.dtype]
            g, w = got[lo:hi], self.want[lo:hi]
            bad = (torch.isnan(g) != torch.isnan(w)) | ((ibits(g) != ibits(w)) & ~torch.isnan(w))
            if bool(bad.any()):
                first = int(bad.nonzero()[0]) - ELEMS[self.dtype]
                raise AssertionError(f'{what}, n = {self.n}, rows = {rows}, out starts {offset} elements past a 16-byte boundary: {int(bad.sum())} wrong, '
                                     f'first at element {first} of the block (row {first // self.n}, column {first % self.n}; negative: the guard before it)')
        raise AssertionError(f'{what}: the buffer changed outside every block and its guards')


@pytest.mark.parametrize('dtype,n', SWEEP, ids=SWEEP_IDS)
def test_gather_at_every_alignment_class(dtype, n):
    """out = the first n columns of the reference for n <= m, +0 from column m on for n > m, NaN all round untouched"""
    E = ELEMS[dtype]
    in_features, nopairs, seed, m = gather_shape(n, E)
    cols, _, scale32 = host_columns(seed, in_features, nopairs)
    assert cols.numel() == m
    rows_of = sweep_rows(n, E)
    x = coded(rows_of[-1], in_features, dtype, 1283)
    ref = gather_reference(x, cols, scale32)
    full = torch.zeros(rows_of[-1], max(n, m), dtype=dtype)
    full[:, :m] = ref
    calls = [(offset, rows) for offset in range(E) for rows in rows_of]
    arena = Arena(dtype, calls, n)
    xd = x.to(DEV)
    for i, (offset, rows) in enumerate(calls):
        got = cabi_x.crs_gather(xd[:rows], seed, nopairs, n, out=arena.out(i))
        assert got.data_ptr() == arena.out(i).data_ptr()
        arena.expect(i, full[:rows, :n])
    arena.check(f'gather {dtype}, m = {m}')


@pytest.mark.parametrize('dtype,n', SWEEP, ids=SWEEP_IDS)
def test_scatter_at_every_alignment_class(dtype, n):
    """gw (n = in_features wide) holds the bits of t[:, j] in column cols[j] for j < cap and +0 everywhere else -- the columns at positions
    >= cap included, when t has fewer columns than the seed has"""
    E = ELEMS[dtype]
    in_features, nopairs, seed = scatter_shape(n)
    cols = host_columns(seed, in_features, nopairs)[0]
    m, caps = scatter_caps(n)
    rows_of = sweep_rows(n, E)
    t_all = coded(rows_of[-1], caps[-1], dtype, 1283)
    calls = [(offset, rows) for offset in range(E) for rows in rows_of]
    arena = Arena(dtype, calls, n)
    td = t_all.to(DEV)
    for i, (offset, rows) in enumerate(calls):
        cap = caps[i % len(caps)]
        cabi_x.crs_scatter(td[:rows, :cap].contiguous(), seed, in_features, nopairs, out=arena.out(i))
        want = torch.zeros(rows, n, dtype=dtype)
        live = min(cap, m)
        want[:, cols[:live]] = t_all[:rows, :live]
        arena.expect(i, want)
    arena.check(f'scatter {dtype}, m = {m}, caps {caps} in turn')


# ---- 2. the columns the device evaluates --------------------------------------------------------------------------------------------------
PREP_IN = (1, 2, 1023, 1024, 1025, 8191, 8192, 8193, 1 << 20)          # one column; the 1024 threads' chunks; LDS / global counters; the maximum
MAX_PAIRS = 1 << 22


def prep_pairs(in_features):
    """the draw loop's steps of 4096 (4 draws x 1024 threads), a ragged last Philox block, four draws per column, one draw per column"""
    return sorted({1, 3, 4, 5, 4095, 4096, 4097, min(4 * in_features, MAX_PAIRS), in_features})


def device_columns_agree(in_features, nopairs, seed):
    cols, count, scale32 = host_columns(seed, in_features, nopairs)
    m, cap = cols.numel(), min(nopairs, in_features)
    assert int(count.sum()) == nopairs
    what = f'in_features = {in_features}, nopairs = {nopairs}, seed = {seed:#x}'
    # pos, whole: the scatter of t[0][j] = j + 1
    t = torch.arange(1, cap + 1, dtype=torch.float32, device=DEV)[None, :]
    want_pos = torch.zeros(1, in_features)
    want_pos[0, cols] = torch.arange(1, m + 1, dtype=torch.float32)
    # scale (and m): the gather of ones
    ones = torch.ones(1, in_features, device=DEV)
    want_scale = torch.zeros(1, cap)
    want_scale[0, :m] = scale32
    for s in (seed, seed_word(seed)):
        form = f'{what}, the seed {"by value" if isinstance(s, int) else "as a device word"}'
        assert_bits(cabi_x.crs_scatter(t, s, in_features, nopairs).cpu(), want_pos, f'pos: {form}')
        assert_bits(cabi_x.crs_gather(ones, s, nopairs, cap).cpu(), want_scale, f'scale: {form}')
    if nopairs == in_features:
        # cols: scale = count exactly, so the gather of x[0][c] = c is cols[j] * count[j] (one rounding where that exceeds 2^24: the reference's)
        assert torch.equal(scale32, count.float())
        ramp = torch.arange(in_features, dtype=torch.float32)[None, :]
        want_cols = torch.zeros(1, cap)
        want_cols[0, :m] = (cols.double() * count.double()).float()
        assert torch.equal(want_cols[:, :m], gather_reference(ramp, cols, scale32))
        for s in (seed, seed_word(seed)):
            assert_bits(cabi_x.crs_gather(ramp.to(DEV), s, nopairs, cap).cpu(), want_cols, f'cols: {what}')


@pytest.mark.parametrize('in_features', PREP_IN)
def test_the_device_evaluates_the_columns_of_the_host(in_features):
    for nopairs in prep_pairs(in_features):
        device_columns_agree(in_features, nopairs, (0x9e3779b97f4a7c15 * (in_features + 31 * nopairs)) & MASK64)


def test_one_column_drawn_four_million_times():
    cols, count, scale32 = host_columns(0xfedcba9876543210, 1, MAX_PAIRS)
    assert cols.tolist() == [0] and count.tolist() == [MAX_PAIRS] and scale32.tolist() == [1.0]
    device_columns_agree(1, MAX_PAIRS, 0xfedcba9876543210)


def test_the_maximum_shape_is_in_the_sweep():
    assert (1 << 20) in PREP_IN and MAX_PAIRS in prep_pairs(1 << 20)


def test_calls_outside_the_range_are_refused_by_name_without_a_launch():
    x = torch.ones(3, 16, device=DEV)
    out = torch.full((3, 8), float('nan'), device=DEV)
    with pytest.raises(cabi.FewbitHipError, match='cap = 0'):
        cabi_x.crs_gather(x, 1, 8, 0)
    with pytest.raises(cabi.FewbitHipError, match='cap = 9'):
        cabi_x.crs_gather(x, 1, 8, 9)
    with pytest.raises(cabi.FewbitHipError, match='cap = 17'):
        cabi_x.crs_gather(x, 1, 64, 17)
    with pytest.raises(cabi.FewbitHipError, match='cap = 9'):                          # scatter: the columns of t
        cabi_x.crs_scatter(torch.ones(3, 9, device=DEV), 1, 16, 8)
    with pytest.raises(cabi.FewbitHipError, match=f'nopairs = {MAX_PAIRS + 1}'):
        cabi_x.crs_gather(x, 1, MAX_PAIRS + 1, 8, out=out)
    with pytest.raises(cabi.FewbitHipError, match=f'nopairs = {MAX_PAIRS + 1}'):
        cabi_x.crs_scatter(torch.ones(3, 8, device=DEV), 1, 16, MAX_PAIRS + 1)
    wide = torch.ones(1, (1 << 20) + 1, device=DEV)
    with pytest.raises(cabi.FewbitHipError, match=f'in_features = {(1 << 20) + 1}'):
        cabi_x.crs_gather(wide, 1, 8, 8, out=out[:1])
    with pytest.raises(cabi.FewbitHipError, match=f'in_features = {(1 << 20) + 1}'):
        cabi_x.crs_scatter(torch.ones(3, 8, device=DEV), 1, (1 << 20) + 1, 8)
    # the library itself says so too (the binding asks its workspace query first): the status of a refusal, the argument in the message
    L, ws = cabi_x.lib(), torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    for cap, in_features, nopairs, name in ((0, 16, 8, b'cap = 0'), (9, 16, 8, b'cap = 9'), (8, (1 << 20) + 1, 8, b'in_features = 1048577'),
                                            (8, 16, MAX_PAIRS + 1, b'nopairs = 4194305')):
        assert L.fewbit_hipx_crs_gather(0, x.data_ptr(), 3, in_features, in_features, 1, None, nopairs, cap, out.data_ptr(), ws.data_ptr(), ws.numel(), None) < 0
        assert name in L.fewbit_hipx_last_error()
        assert L.fewbit_hipx_crs_scatter(0, x.data_ptr(), 3, cap, 1, None, in_features, nopairs, out.data_ptr(), ws.data_ptr(), ws.numel(), None) < 0
        assert name in L.fewbit_hipx_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                                                # nothing ran


# ---- 3. values ------------------------------------------------------------------------------------------------------------------------
VALUE_SHAPE = (8, 24, 0xed9e0001)           # in_features, nopairs, seed: scales are multiples of 1 / 3


def value_columns():
    """the columns of VALUE_SHAPE: one drawn once (scale 1/3), one twice (2/3), one five times (5/3), asserted"""
    in_features, nopairs, seed = VALUE_SHAPE
    cols, count, scale32 = host_columns(seed, in_features, nopairs)
    assert 1 in count.tolist() and 2 in count.tolist() and 5 in count.tolist() and max(count.tolist()) >= 2, count.tolist()
    return cols, count, scale32


def all_patterns(dtype):
    """65536 x 8: x[r][c] = the 16-bit pattern (r + 8192 c) mod 65536 -- every column holds every pattern"""
    r, c = torch.arange(65536, dtype=torch.int64)[:, None], torch.arange(8, dtype=torch.int64)[None, :]
    pattern = (r + 8192 * c) % 65536
    return torch.where(pattern >= 32768, pattern - 65536, pattern).to(torch.int16).view(dtype)


def fp32_specials():
    """one fp32 column: zeros, infinities, NaNs (payloads, negative), the ends of the normal and subnormal ranges, values whose product with
    fl(1/3) or fl(5/3) is an exact tie between two subnormal-spaced results, the 4096 patterns nearest to a tie of either product among
    2^20 random ones, and 4096 random patterns"""
    words = [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 0x7fa00000, 0x7f7fffff, 0xff7fffff,
             0x00800000, 0x80800000, 0x00800001, 0x007fffff, 0x807fffff, 0x00000001, 0x80000001, 0x00000002, 0x00000003, 0x00400000, 0x00c00000,
             0x3f800000, 0xbf800000, 0x40400000, 0x3eaaaaab, 0x3fd55555]
    special = torch.tensor(words, dtype=torch.int64)
    # fl(5/3) = 13981013 x 2^-23 and fl(1/3) = 11184811 x 2^-25 are odd multiples: k x 2^-127 x fl(5/3) and k x 2^-125 x fl(1/3), k odd, are
    # odd multiples of 2^-150, half a step of the results below 2^-125
    third, five_thirds = torch.tensor(1 / 3, dtype=torch.float64).float(), torch.tensor(5 / 3, dtype=torch.float64).float()
    ties = []
    for k in (1, 3, 5, 7, 9, 11):
        for v in (k * 2.0**-127, k * 2.0**-125):
            ties += [v, -v]
    ties = torch.tensor(ties, dtype=torch.float64).float()
    for v in ties[0::4]:
        assert float(v.double() * five_thirds.double() * 2.0**149) % 1.0 == 0.5
    for v in ties[2::4]:
        assert float(v.double() * third.double() * 2.0**149) % 1.0 == 0.5
    g = torch.Generator().manual_seed(20)
    pool = torch.randint(-2**31, 2**31, (1 << 20, ), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    pool = pool[torch.isfinite(pool) & (pool.abs() > 2.0**-100) & (pool.abs() < 2.0**100)]
    near = []
    for s in (third, five_thirds):
        p = pool.double() * s.double()
        step = torch.ldexp(torch.ones_like(p), torch.frexp(p)[1] - 24)                  # the fp32 step at p
        frac = torch.remainder(p / step, 1.0)
        near.append(pool[torch.argsort((frac - 0.5).abs())[:2048]])
    rand = torch.randint(-2**31, 2**31, (4096, ), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    head = torch.where(special >= 2**31, special - 2**32, special).to(torch.int32).view(torch.float32)
    return torch.cat([head, ties, *near, rand])


@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float16))
def test_gather_rounds_every_16_bit_pattern_as_the_reference_does(dtype):
    """+-0 (the sign kept), subnormals, the largest finite values (fp16: past the range under 5/3), +-inf, every NaN, every tie of both
    roundings, under scales 1/3 .. 5/3.  (fl(5/3) x is where a product rounded ONCE to fp16 -- one fused multiply-and-convert instruction -- ends one step
    below the contract's fp32 product rounded to fp16, on 6 % of the patterns: the fp16 kernel did that until this test ran.)"""
    in_features, nopairs, seed = VALUE_SHAPE
    cols, count, scale32 = value_columns()
    x = all_patterns(dtype)
    want = gather_reference(x, cols, scale32)
    if dtype == torch.float16:
        assert bool(torch.isinf(want[torch.isfinite(x.float()[:, cols])]).any())        # the overflow by the scale is in the data
    got = cabi_x.crs_gather(x.to(DEV), seed, nopairs).cpu()
    assert_gathered(got, want, f'gather of every {dtype} pattern, counts {count.tolist()}')
    assert_gathered(cabi_x.crs_gather(x.to(DEV), seed_word(seed), nopairs).cpu()[:, :cols.numel()], want, f'the same, the seed as a device word')


def test_gather_multiplies_fp32_as_the_reference_does():
    in_features, nopairs, seed = VALUE_SHAPE
    cols, count, scale32 = value_columns()
    vals = fp32_specials()
    x = torch.stack([vals.roll(37 * c) for c in range(in_features)], dim=1).contiguous()
    want = gather_reference(x, cols, scale32)
    small = (want != 0) & (want.abs() < 2.0**-126)
    assert bool(small.any()) and bool(torch.isnan(want).any()) and bool(torch.isinf(want[torch.isfinite(x[:, cols])]).any())
    got = cabi_x.crs_gather(x.to(DEV), seed, nopairs).cpu()
    assert_gathered(got, want, f'gather of the fp32 specials, counts {count.tolist()}')


@pytest.mark.parametrize('dtype', DTYPES)
def test_scatter_copies_every_bit_pattern(dtype):
    """gw[:, cols] carries the bits of t -- NaN payloads, negative NaN, -0, subnormals -- and everything else is +0"""
    in_features, nopairs, seed = VALUE_SHAPE
    cols, _, _ = value_columns()
    m = cols.numel()
    if dtype == torch.float32:
        vals = fp32_specials()
        t = torch.stack([vals.roll(37 * j) for j in range(m)], dim=1).contiguous()
    else:
        t = all_patterns(dtype)[:, :m].contiguous()
    want = torch.zeros(t.shape[0], in_features, dtype=dtype)
    want[:, cols] = t
    assert_bits(want[:, cols], t, 'the host image')                                     # (the host copy keeps the bits too)
    assert_bits(cabi_x.crs_scatter(t.to(DEV), seed, in_features, nopairs).cpu(), want, f'scatter of every {dtype} pattern')


# ---- 4. the layer against float64 ---------------------------------------------------------------------------------------------------------
LAYER_SEED = 0x3c6ef372fe94f82b
ROWS, IN, OUT = 256, 96, 40
VARIANTS = ('2-D', '3-D', 'row-strided', 'feature-strided', 'no bias', 'input without gradient')


def weight_gradient_check(gw, x, gy, seed, nopairs, what):
    """gw: the layer's weight gradient (device); x, gy: what the layer saw (any shape, device).  -> worst |err| / bound over the drawn columns

        |gw[:, cols] - want| <= u_out |want| + (rows + 2) 2^-24 bound (+ 2^-24 for fp16),  want = G64^T kept64,  bound = |G64|^T |kept64|

    kept: the gather's reference.  The library GEMM accumulates in fp32 and rounds once to the dtype: the standard dot-product bound for any
    summation order (fp32 inputs add one rounding per product, 16-bit products are exact in fp32).  Outside cols: +0 bit for bit."""
    dtype, in_features = gw.dtype, gw.shape[1]
    flat, gflat = x.detach().reshape(-1, in_features).cpu(), gy.detach().reshape(-1, gy.shape[-1]).cpu()
    rows = flat.shape[0]
    cols, _, scale32 = host_columns(seed, in_features, nopairs)
    kept = gather_reference(flat.contiguous(), cols, scale32).double()
    g64 = gflat.double()
    want, bound = g64.T @ kept, g64.abs().T @ kept.abs()
    tol = U_OUT[dtype] * want.abs() + (rows + 2) * 2.0**-24 * bound + (2.0**-24 if dtype == torch.float16 else 0.0)
    got = gw.detach().cpu()
    err = (got[:, cols].double() - want).abs()
    ratio = float((err / tol.clamp_min(1e-300)).max())
    rest = torch.ones(in_features, dtype=torch.bool)
    rest[cols] = False
    assert not bool(ibits(got[:, rest]).any()), (what, 'an entry outside the drawn columns is not +0')
    assert bool(torch.isfinite(got).all()) and int(torch.count_nonzero(got[:, cols])) > 0, what
    print(f'crs edges: {what}: worst err / bound = {ratio:.4f}')
    assert bool((err <= tol).all()), (what, f'worst err / bound = {ratio:.4f}', float(err.max()))
    return ratio


def layer_inputs(dtype, variant):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(ROWS, IN, generator=g).to(dtype).to(DEV)
    w, b, gy = (torch.randn(s, generator=g).to(dtype).to(DEV) for s in ((OUT, IN), (OUT, ), (ROWS, OUT)))
    if variant == '3-D':
        x, gy = x.reshape(2, ROWS // 2, IN), gy.reshape(2, ROWS // 2, OUT)
    elif variant == 'row-strided':
        buf = torch.full((ROWS, 104), float('nan'), dtype=dtype, device=DEV)
        buf[:, :IN] = x
        x = buf[:, :IN]
        assert x.stride() == (104, 1)
    elif variant == 'feature-strided':
        buf = torch.full((ROWS, 2 * IN), float('nan'), dtype=dtype, device=DEV)
        buf[:, ::2] = x
        x = buf[:, ::2]
        assert x.stride() == (2 * IN, 2)
    return x, w, (None if variant == 'no bias' else b), gy


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_the_layer_against_float64(dtype, variant, monkeypatch):
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: LAYER_SEED)
    x, w, b, gy = layer_inputs(dtype, variant)
    for nopairs in (1, 48, 384):
        xi = x.detach().requires_grad_(variant != 'input without gradient')
        wi = w.clone().requires_grad_()
        bi = None if b is None else b.clone().requires_grad_()
        y = fewbit.functional.linear_crs(xi, wi, bi, nopairs)
        y.backward(gy)
        weight_gradient_check(wi.grad, x, gy, LAYER_SEED, nopairs, f'layer {dtype}, {variant}, nopairs = {nopairs}')
        # everything but the weight gradient is F.linear's
        assert torch.equal(y.detach(), F.linear(x, w, b))
        if xi.requires_grad:
            assert torch.equal(xi.grad, gy @ w)
        else:
            assert xi.grad is None
        if bi is not None:
            assert torch.equal(bi.grad, gy.reshape(-1, OUT).sum(dim=0))


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_second_backward_adds_exactly_the_first_and_the_weight_alone_gets_the_same_bits(dtype, monkeypatch):
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: LAYER_SEED)
    x, w, b, gy = layer_inputs(dtype, '2-D')
    for nopairs in (1, 48, 384):
        xi, wi, bi = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        y = fewbit.functional.linear_crs(xi, wi, bi, nopairs)
        y.backward(gy, retain_graph=True)
        first = [t.grad.clone() for t in (xi, wi, bi)]
        y.backward(gy)
        for once, t in zip(first, (xi, wi, bi)):
            assert_bits(t.grad.cpu(), (once + once).cpu(), f'{dtype}, nopairs = {nopairs}: the second pass')
        assert int(torch.count_nonzero(first[1])) > 0
        alone = w.clone().requires_grad_()
        fewbit.functional.linear_crs(x, alone, b, nopairs).backward(gy)
        assert_bits(alone.grad.cpu(), first[1].cpu(), f'{dtype}, nopairs = {nopairs}: only the weight needs a gradient')


# ---- 5. several randomized layers in one captured step --------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float32))
def test_every_layer_of_a_captured_step_meets_its_own_seed_in_backward(dtype, monkeypatch):
    """LinearCRS(64, 96) -> GELU(bits=3) -> RandomizedLinear(96, 64, 'rademacher', 0.25) -> LinearCRS(64, 32) on 512 rows, forward and backward in
    ONE graph.  While capturing, every seeded layer records a seed kernel: word = mix(base of the layer's host draw, counter), counter += 1,
    in forward order; so replay r gives layer l (of L = 3) the seed mix_sketch_seed(base_l, c0 + L r + l), and its backward -- which runs
    after the other layers drew theirs -- must meet that word, not a neighbour's.  The inputs and gradients the layers saw are kept as
    outputs of the graph (hooks on the intermediate tensors)."""
    rows, L = 512, 3
    torch.manual_seed(5)
    l1 = fewbit.LinearCRS(64, 96, device=DEV, dtype=dtype)
    act = fewbit.GELU(bits=3)
    l3 = fewbit.RandomizedLinear(96, 64, matmul='rademacher', proj_dim_ratio=0.25, device=DEV, dtype=dtype)
    l4 = fewbit.LinearCRS(64, 32, device=DEV, dtype=dtype)
    p = int(0.25 * rows)
    x = torch.randn(rows, 64, device=DEV).to(dtype)
    gy = torch.randn(rows, 32, device=DEV).to(dtype)
    weights = [l1.weight, l3.weight, l4.weight]
    kept = {}

    def step():
        h1 = l1(x)
        h1.register_hook(lambda g: kept.__setitem__('g1', g))                          # dL/dh1: what l1's backward is given
        h2 = act(h1)                                                                    # (in place on h1: the hook above belongs to the value before)
        h3 = l3(h2)
        h3.register_hook(lambda g: kept.__setitem__('g3', g))
        h4 = l4(h3)
        kept['h2'], kept['h3'] = h2, h3
        return torch.autograd.grad(h4, weights, gy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    bases = []

    def draw(generator):
        bases.append(0x1234567 + 0x1000193 * len(bases))
        return bases[-1]

    monkeypatch.setattr(linear, '_draw_seed', draw)
    counter = linear._replay_counter(torch.device(DEV))
    c0 = int(counter)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        grads = step()
    assert len(bases) == L and len(set(bases)) == L and int(counter) == c0            # three host draws at capture time; recording runs nothing
    seen = []
    for r in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert int(counter) == c0 + L * (r + 1)
        seeds = [cabi.mix_sketch_seed(bases[l], c0 + L * r + l) for l in range(L)]
        assert len(set(seeds)) == L
        weight_gradient_check(grads[0], x, kept['g1'], seeds[0], l1.nopairs, f'captured {dtype}, replay {r}, LinearCRS(64, 96)')
        weight_gradient_check(grads[2], kept['h3'], gy, seeds[2], l4.nopairs, f'captured {dtype}, replay {r}, LinearCRS(64, 32)')
        # the Rademacher layer: the eager products of the same seed
        pg, px = cabi.sketch('rademacher', kept['g3'].contiguous(), p, seeds[1]), cabi.sketch('rademacher', kept['h2'].detach(), p, seeds[1], 1.0 / p)
        if dtype == torch.float32:
            want = pg.T @ px
            assert torch.allclose(grads[1], want, rtol=1e-4, atol=1e-3), (r, float((grads[1] - want).abs().max()))
        else:
            # two GEMMs of the same 16-bit operands may sum in different orders: each is within the bound of part 4 of the float64 product
            want, bound = pg.double().T @ px.double(), pg.double().abs().T @ px.double().abs()
            tol = U_OUT[dtype] * want.abs() + (p + 2) * 2.0**-24 * bound
            err = (grads[1].double() - want).abs()
            print(f'crs edges: captured {dtype}, replay {r}, RandomizedLinear: worst err / bound = {float((err / tol.clamp_min(1e-300)).max()):.4f}')
            assert bool((err <= tol).all()), (r, float((err / tol.clamp_min(1e-300)).max()))
        seen.append([t.clone() for t in grads])
    for l in range(L):
        assert not torch.equal(seen[0][l], seen[1][l]) and not torch.equal(seen[1][l], seen[2][l]) and not torch.equal(seen[0][l], seen[2][l]), l
