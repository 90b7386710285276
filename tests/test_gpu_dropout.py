"""The dropout of a seed on the GPU (fewbit_amd/csrc/fewbit_dropout.hip).  Every reference is computed on the HOST: the mask from
``cabi_x.dropout_keep`` (the host evaluation of the definition in include/fewbit_hipx.h), the arithmetic by torch's host operators,

    want = torch.where(keep, x.float() * scale32 [+ r.float()], r.float() or 0).to(dtype)          scale32 = float32(65536 / (65536 - T))

(the product and the sum each rounded to fp32, one rounding to the dtype) and compared bit for bit; NaN is compared by position (the bits of
a NaN are not part of the contract: a bf16 NaN result is the canonical 0x7fc0)."""
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
ONE = 65536
THRESHOLDS = (1, 6554, 32768, 65535)
# one sweep of the launch plan covers cabi_x.DROPOUT_SWEEP elements: one more makes the first lane take a second block
SIZES = (1, 7, 8, 9, 63, 64, 65, 4095, 4096, 4097, 2**20 + 3, cabi_x.DROPOUT_SWEEP + 1 + 3)
SENTINEL, GUARD = 123.0, 64
SEED = 0x1234567887654321


@pytest.fixture(autouse=True)
def native_sketch_on():
    prev = linear.use_native_sketch(True)
    yield
    linear.use_native_sketch(prev)


@functools.lru_cache(maxsize=32)
def host_keep(seed, n, threshold, first=0):
    return cabi_x.dropout_keep(seed, n, threshold / ONE, first)


def scale32(threshold):
    return torch.tensor(65536.0 / (ONE - threshold), dtype=torch.float64).float()


def reference(x, r, keep, threshold):
    """x, r (or None): host tensors of the kernel's dtype"""
    kept = x.float() * scale32(threshold)
    if r is not None:
        kept = kept + r.float()
    return torch.where(keep, kept, torch.zeros_like(kept) if r is None else r.float()).to(x.dtype)


def specials(dtype):
    fi = torch.finfo(dtype)
    return (0.0, -0.0, float('inf'), -float('inf'), float('nan'), fi.max, -fi.max, fi.smallest_normal * fi.eps, -fi.smallest_normal * fi.eps)


@functools.lru_cache(maxsize=8)
def values(n, dtype, salt):
    """n host values of `dtype`: normal draws with the specials of the dtype at 9 of every 64 positions (rotated by `salt`)"""
    g = torch.Generator().manual_seed(1000 + salt)
    x = (torch.randn(n, generator=g) * 3).to(dtype)
    sp = specials(dtype)
    for k in range(len(sp)):
        x[k::64] = sp[(k + salt) % len(sp)]
    return x


def placed(t, offset):
    """-> (buffer, view): `t` on the device inside a buffer of sentinels, `offset` elements from its 16-byte aligned start and GUARD before its end"""
    buf = torch.full((offset + t.numel() + GUARD, ), SENTINEL, dtype=t.dtype, device=DEV)
    view = buf[offset:offset + t.numel()]
    view.copy_(t)
    assert view.data_ptr() % 16 == (offset * t.element_size()) % 16
    return buf, view


def assert_same(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), (what, 'NaN in other places', int((torch.isnan(got) != nan).sum()))
    bad = (got.view(INT[got.dtype]) != want.view(INT[want.dtype])) & ~nan
    if bool(bad.any()):
        at = bad.nonzero().flatten()[:6].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} differ, first at {at}: got {got[at].tolist()}, want {want[at].tolist()}')


def assert_guards(buf, offset, n, what):
    assert bool((buf[:offset] == SENTINEL).all()) and bool((buf[offset + n:] == SENTINEL).all()), f'{what}: written outside the {n} elements'


# ---- 1. bit-exact forward, bounds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: str(d).split('.')[-1])
def test_forward_is_bit_exact_and_stays_inside(dtype, n):
    x, r = values(n, dtype, 0), values(n, dtype, 3)
    # (at the two large sizes: every threshold and both addend cases on aligned pointers, one threshold on offset ones)
    for threshold in THRESHOLDS:
        keep = host_keep(SEED, n, threshold)
        for addend in (None, r):
            want = reference(x, addend, keep, threshold)
            for offset in (0, 1):
                if n > 4097 and offset and threshold != 6554:
                    continue
                what = f'{dtype} n = {n} T = {threshold} addend = {addend is not None} offset = {offset}'
                _, xd = placed(x, offset)
                rd = None if addend is None else placed(addend, offset)[1]
                obuf, od = placed(torch.full_like(x, SENTINEL), offset)
                got = cabi_x.dropout_apply(xd, SEED, threshold / ONE, rd, out=od)
                assert got is od
                assert_same(od, want, what)
                assert_guards(obuf, offset, n, what)
                assert_same(xd, x, what + ' (src)')


@pytest.mark.parametrize('n', (9, 4097))
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: str(d).split('.')[-1])
def test_out_may_be_src_or_addend(dtype, n):
    x, r, threshold = values(n, dtype, 1), values(n, dtype, 5), 32768
    keep = host_keep(SEED, n, threshold)
    for offset in (0, 1):
        for addend in (None, r):
            want, what = reference(x, addend, keep, threshold), f'{dtype} n = {n} addend = {addend is not None} offset = {offset}'
            xbuf, xd = placed(x, offset)
            rd = None if addend is None else placed(addend, offset)[1]
            cabi_x.dropout_apply(xd, SEED, threshold / ONE, rd, out=xd)
            assert_same(xd, want, what + ', out is src')
            assert_guards(xbuf, offset, n, what)
        _, xd = placed(x, offset)
        rbuf, rd = placed(r, offset)
        cabi_x.dropout_apply(xd, SEED, threshold / ONE, rd, out=rd)
        assert_same(rd, reference(x, r, keep, threshold), f'{dtype} n = {n} offset = {offset}, out is addend')
        assert_guards(rbuf, offset, n, 'out is addend')


def test_allocated_output_and_the_extremes_of_the_threshold():
    x = values(1000, torch.bfloat16, 2).to(DEV)
    same = cabi_x.dropout_apply(x, SEED, 0.0)
    assert_same(same, x.cpu().float().mul(1.0).to(torch.bfloat16), 'T = 0')              # scale 1: the values (a NaN stays a NaN)
    none = cabi_x.dropout_apply(x, SEED, 1.0)
    assert none.shape == x.shape and bool((none.view(torch.int16) == 0).all())           # T = 65536: +0 everywhere, inf and NaN included
    r = values(1000, torch.bfloat16, 4).to(DEV)
    assert torch.equal(cabi_x.dropout_apply(x, SEED, 1.0, r).view(torch.int16), r.view(torch.int16))
    assert cabi_x.dropout_apply(x[:0], SEED, 0.5).numel() == 0
    with pytest.raises(cabi.FewbitHipError, match='multiple of 8'):
        cabi_x.dropout_apply(x, SEED, 0.5, first=4)
    with pytest.raises(cabi.FewbitHipError, match='contiguous'):
        cabi_x.dropout_apply(x[::2], SEED, 0.5)


# ---- 2. `first`: a buffer anywhere in a logical tensor ---------------------------------------------------------------------------------
@pytest.mark.parametrize('first', (8, 2**35, 2**35 - 24))
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: str(d).split('.')[-1])
def test_first_on_the_device(dtype, first):
    """64 elements from `first` (from 2^35 - 24: the carry into counter word 1 falls inside the launch)"""
    n, threshold = 64, 32768
    x = (torch.arange(n) + 1).to(dtype)
    for seed in (SEED, torch.tensor([SEED], dtype=torch.int64, device=DEV)):
        got = cabi_x.dropout_apply(x.to(DEV), seed, threshold / ONE, first=first)
        assert_same(got, reference(x, None, host_keep(SEED, n, threshold, first), threshold), f'{dtype} first = {first}')
    assert not torch.equal(host_keep(SEED, n, threshold, first), host_keep(SEED, n, threshold, 0))


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: str(d).split('.')[-1])
def test_two_halves_give_the_bytes_of_the_whole(dtype):
    n, p = 4096 + 16, 0.1
    x, r = values(n, dtype, 6).to(DEV), values(n, dtype, 7).to(DEV)
    whole = cabi_x.dropout_apply(x, SEED, p, r)
    half = n // 2
    parts = torch.cat((cabi_x.dropout_apply(x[:half], SEED, p, r[:half]), cabi_x.dropout_apply(x[half:], SEED, p, r[half:], first=half)))
    assert torch.equal(parts.view(INT[dtype]), whole.view(INT[dtype]))


# ---- 3. the layer --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def seeds(monkeypatch):
    """the seeds the layer draws, in order"""
    drawn = []
    real = linear._draw_seed

    def draw(generator):
        drawn.append(real(generator))
        return drawn[-1]

    monkeypatch.setattr(linear, '_draw_seed', draw)
    return drawn


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: str(d).split('.')[-1])
def test_backward_uses_the_forwards_mask_and_saves_nothing(dtype, seeds):
    shape, p = (37, 129), 0.1
    n, threshold = 37 * 129, 6554
    torch.manual_seed(0)
    x = torch.randn(shape, dtype=dtype, device=DEV, requires_grad=True)
    gy = torch.randn(shape, dtype=dtype, device=DEV)
    with fewbit.memory_usage_hooks() as usage:
        y = fewbit.functional.dropout(x, p)
    assert not usage.forward and len(seeds) == 1 and y.shape == x.shape and y.is_contiguous()
    keep = host_keep(seeds[0], n, threshold).view(shape)
    assert_same(y.detach(), reference(x.detach().cpu(), None, keep, threshold), f'{dtype} forward')
    y.backward(gy)
    assert_same(x.grad, reference(gy.cpu(), None, keep, threshold), f'{dtype} backward')
    with fewbit.memory_usage_hooks() as torch_usage:
        F.dropout(x, p)
    assert torch_usage.forward == n                                    # one bool per element
    # the module is the function
    m = fewbit.Dropout(p)
    ym = m(x)
    assert len(seeds) == 2 and ym.grad_fn is not None
    assert_same(ym.detach(), reference(x.detach().cpu(), None, host_keep(seeds[1], n, threshold).view(shape), threshold), 'module')
    assert m.eval()(x) is x and len(seeds) == 2
    # p = 1: zeros, and a zero gradient
    x.grad = None
    z = fewbit.functional.dropout(x, 1.0)
    z.backward(gy)
    assert bool((z == 0).all()) and bool((x.grad == 0).all())


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: str(d).split('.')[-1])
def test_dropout_add(dtype, seeds):
    shape, p, threshold = (5, 7, 33), 0.5, 32768
    n = 5 * 7 * 33
    torch.manual_seed(1)
    x = torch.randn(shape, dtype=dtype, device=DEV, requires_grad=True)
    r = torch.randn(shape, dtype=dtype, device=DEV, requires_grad=True)
    gy = torch.randn(shape, dtype=dtype, device=DEV)
    with fewbit.memory_usage_hooks() as usage:
        y = fewbit.functional.dropout_add(x, r, p)
    assert not usage.forward and len(seeds) == 1
    keep = host_keep(seeds[0], n, threshold).view(shape)
    assert_same(y.detach(), reference(x.detach().cpu(), r.detach().cpu(), keep, threshold), f'{dtype} forward')
    y.backward(gy)
    assert torch.equal(r.grad, gy)
    assert_same(x.grad, reference(gy.cpu(), None, keep, threshold), f'{dtype} backward')
    # only the residual wants a gradient; unequal shapes broadcast through the composed form
    y = fewbit.functional.dropout_add(x.detach(), r, p)
    (gr, ) = torch.autograd.grad(y, r, gy)
    assert torch.equal(gr, gy)
    row = torch.randn(33, dtype=dtype, device=DEV)
    y = fewbit.functional.dropout_add(x.detach(), row, p)
    keep = host_keep(seeds[-1], n, threshold).view(shape)
    assert_same(y, row.cpu() + reference(x.detach().cpu(), None, keep, threshold), 'broadcast residual')
    assert torch.equal(fewbit.functional.dropout_add(x, r, p, training=False), r + x)


def test_seeds_reproduce_and_calls_differ():
    x = torch.ones(4096, device=DEV)
    torch.manual_seed(11)
    a, b = fewbit.functional.dropout(x, 0.5), fewbit.functional.dropout(x, 0.5)
    torch.manual_seed(11)
    a2 = fewbit.functional.dropout(x, 0.5)
    assert torch.equal(a, a2) and not torch.equal(a, b)
    # a device generator is accepted (its offset moves, the host generator does not)
    gen = torch.Generator(device=DEV).manual_seed(5)
    before = torch.get_rng_state()
    c, d = fewbit.functional.dropout(x, 0.5, generator=gen), fewbit.functional.dropout(x, 0.5, generator=gen)
    assert torch.equal(torch.get_rng_state(), before) and not torch.equal(c, d)
    assert torch.equal(c, fewbit.functional.dropout(x, 0.5, generator=torch.Generator(device=DEV).manual_seed(5)))
    host = torch.Generator().manual_seed(6)
    e = fewbit.Dropout(0.5, generator=host)(x)
    assert torch.equal(e, fewbit.functional.dropout(x, 0.5, generator=torch.Generator().manual_seed(6)))


def test_layouts_inplace_no_grad_and_the_switch(seeds):
    threshold = 32768
    base = torch.randn(24, 40, device=DEV)
    # a non-contiguous input: gathered, the output contiguous; the gradient arrives in the input's layout
    xt = base.t().requires_grad_()
    y = fewbit.functional.dropout(xt, 0.5)
    assert y.is_contiguous() and y.shape == xt.shape
    keep = host_keep(seeds[-1], 960, threshold).view(40, 24)
    assert_same(y.detach(), reference(base.t().contiguous().cpu(), None, keep, threshold), 'transposed input')
    gy = torch.randn(24, 40, device=DEV).t()                          # a non-contiguous gradient
    y.backward(gy)
    assert_same(xt.grad.contiguous(), reference(gy.contiguous().cpu(), None, keep, threshold), 'transposed gradient')
    # in place on a non-leaf
    leaf = torch.randn(1000, device=DEV, requires_grad=True)
    h = leaf * 2
    values_before = h.detach().clone()
    out = fewbit.functional.dropout(h, 0.5, inplace=True)
    assert out.data_ptr() == h.data_ptr() and out._version == h._version > 0
    keep = host_keep(seeds[-1], 1000, threshold)
    assert_same(h.detach(), reference(values_before.cpu(), None, keep, threshold), 'in place')
    h.sum().backward()
    assert_same(leaf.grad, torch.where(keep, 4.0, 0.0), 'gradient through the in-place call')
    with pytest.raises(RuntimeError):
        fewbit.functional.dropout(leaf, 0.5, inplace=True)            # a leaf that requires grad, as in torch
    assert torch.equal(leaf.detach() * 2, values_before)              # (refused before anything was written)
    # in place on a non-contiguous tensor
    plain = torch.randn(24, 40, device=DEV)
    view, was = plain.t(), plain.t().clone()
    fewbit.functional.dropout(view, 0.5, inplace=True)
    assert_same(view.contiguous(), reference(was.contiguous().cpu(), None, host_keep(seeds[-1], 960, threshold).view(40, 24), threshold), 'in place, transposed')
    # no_grad: still dropout, no node
    count = len(seeds)
    with torch.no_grad():
        y = fewbit.Dropout(0.5)(leaf)
    assert y.grad_fn is None and not y.requires_grad and len(seeds) == count + 1 and bool((y == 0).any())
    # float64 and the switch: torch's dropout, which saves its mask
    prev = linear.use_native_sketch(False)
    try:
        with fewbit.memory_usage_hooks() as usage:
            torch.manual_seed(3)
            y = fewbit.functional.dropout(leaf, 0.5)
        torch.manual_seed(3)
        assert usage.forward == 1000 and len(seeds) == count + 1 and torch.equal(y, F.dropout(leaf, 0.5))
    finally:
        linear.use_native_sketch(prev)
    with fewbit.memory_usage_hooks() as usage:
        fewbit.functional.dropout(leaf.double(), 0.5)
    assert usage.forward == 1000 and len(seeds) == count + 1


# ---- 4. graph capture --------------------------------------------------------------------------------------------------------------------
def test_a_captured_step_draws_a_fresh_mask_on_every_replay(monkeypatch):
    n, p, threshold = 2**20, 0.1, 6554
    x = (torch.rand(n, device=DEV) + 0.5).requires_grad_()
    gy = torch.rand(n, device=DEV) + 0.5

    def step():
        y = fewbit.functional.dropout(x, p)
        return y, torch.autograd.grad(y, x, gy)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                        # the eager warm-up: the per-device replay counter exists from here on
    torch.cuda.current_stream().wait_stream(side)
    bases = []
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: bases.append(0x7654321) or bases[-1])
    counter = linear._replay_counter(torch.device(DEV))
    c0 = int(counter)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y, gx = step()
    assert len(bases) == 1 and int(counter) == c0
    sd, drops = (n * (threshold / ONE) * (1 - threshold / ONE))**0.5, []
    for replay in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert int(counter) == c0 + replay + 1
        dropped = y == 0
        assert torch.equal(gx == 0, dropped)                          # backward met its forward's mask
        assert abs(int(dropped.sum()) - n * threshold / ONE) <= 5 * sd
        keep = host_keep(cabi.mix_sketch_seed(bases[0], c0 + replay), n, threshold)
        assert torch.equal(~dropped.cpu(), keep)                      # and it is the mask of the seed the replay counter gave
        drops.append(dropped.clone())
    assert not torch.equal(drops[0], drops[1]) and not torch.equal(drops[1], drops[2]) and not torch.equal(drops[0], drops[2])
