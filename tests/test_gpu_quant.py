"""The packed form of a seed on the GPU (fewbit_amd/csrc/fewbit_quant.hip through cabi_x.quant_pack / quant_unpack).  Every reference is
computed on the HOST: the packed bytes by ``cabi_x.quant_pack_host`` (the host evaluation of the definition in include/fewbit_hipx.h, itself
pinned to a numpy restatement by tests/test_quant_host.py), the decode by ``cabi_x.quant_unpack_host`` rounded once by torch's host
conversion.  Bytes are compared bit for bit; a decoded NaN is compared by position."""
import functools

import pytest
import torch

from fewbit_amd import cabi, cabi_x, linear

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
INT = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
BITS = (2, 4, 8)
# one sweep of the launch plan covers cabi_x.QUANT_SWEEP elements: one block more makes the first lane take a second block, and 3 ragged
# elements behind it the second lane a short one
SIZES = (1, 7, 8, 9, 63, 64, 65, 205, 2573, cabi_x.QUANT_SWEEP + 8 + 3)
SEED = 0x1234567887654321
GUARD, SENTINEL = 16, 0xA5
ids = lambda d: str(d).split('.')[-1]


@functools.lru_cache(maxsize=8)
def values(n, dtype, salt=0):
    g = torch.Generator().manual_seed(2000 + salt)
    return (torch.randn(n, generator=g) * 3).to(dtype)


@functools.lru_cache(maxsize=32)
def host_pack(n, dtype, bits, salt=0, seed=SEED):
    return cabi_x.quant_pack_host(values(n, dtype, salt).float(), seed, bits)


def placed(t, offset):
    """`t` on the device, `offset` elements from the 16-byte aligned start of its buffer"""
    buf = torch.zeros(offset + t.numel() + 8, dtype=t.dtype, device=DEV)
    view = buf[offset:offset + t.numel()]
    view.copy_(t)
    assert view.data_ptr() % 16 == (offset * t.element_size()) % 16
    return view


def guarded_bytes(count, extra=0):
    """-> (buffer of sentinels, its view of `count + extra` bytes behind GUARD bytes)"""
    buf = torch.full((GUARD + count + extra + GUARD, ), SENTINEL, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + count + extra]


def assert_bytes(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, what
    bad = got != want
    if bool(bad.any()):
        at = bad.nonzero().flatten()[:8].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} bytes differ, first at {at}: got {got[at].tolist()}, want {want[at].tolist()}')


def assert_values(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), (what, 'NaN in other places')
    bad = (got.view(INT[got.dtype]) != want.view(INT[want.dtype])) & ~nan
    if bool(bad.any()):
        at = bad.nonzero().flatten()[:6].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} differ, first at {at}: got {got[at].tolist()}, want {want[at].tolist()}')


# ---- 1. pack -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('dtype', DTYPES, ids=ids)
def test_pack_equals_the_host_evaluation_bit_for_bit(dtype, bits, n):
    x, want = values(n, dtype), host_pack(n, dtype, bits)
    need = cabi_x.quant_bytes(n, bits)
    for offset in (0, 1):                                             # 16-byte loads; the element path of an unaligned source
        what = f'{dtype} bits {bits} n {n} offset {offset}'
        xd = placed(x, offset)
        buf, out = guarded_bytes(need, extra=8 * offset)              # (a longer buffer: only the first `need` bytes are the call's)
        got = cabi_x.quant_pack(xd, SEED, bits, out=out)
        assert got is out
        assert_bytes(out[:need], want, what)
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + need:] == SENTINEL).all()), f'{what}: written outside the {need} bytes'
        assert torch.equal(xd.cpu().view(INT[dtype]), x.view(INT[dtype])), f'{what}: src changed'
    again = cabi_x.quant_pack(placed(x, 0), SEED, bits)               # allocated by the call; the same arguments, the same bytes
    assert again.shape == (need, ) and again.dtype == torch.uint8
    assert_bytes(again, want, 'allocated out')
    word = torch.tensor([SEED], dtype=torch.int64, device=DEV)        # the seed as a device word
    assert_bytes(cabi_x.quant_pack(placed(x, 0), word, bits), want, 'seed word')


@pytest.mark.parametrize('bits', BITS)
def test_the_packed_form_does_not_depend_on_the_source_dtype(bits):
    n = 2573
    x = values(n, torch.bfloat16)                                     # bf16 values are fp16-inexact in general: widen to fp32 only
    assert_bytes(cabi_x.quant_pack(x.float().to(DEV), SEED, bits), cabi_x.quant_pack(x.to(DEV), SEED, bits), 'bf16 against its fp32 copy')
    h = values(n, torch.float16)
    assert_bytes(cabi_x.quant_pack(h.float().to(DEV), SEED, bits), cabi_x.quant_pack(h.to(DEV), SEED, bits), 'fp16 against its fp32 copy')


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('dtype', DTYPES, ids=ids)
def test_poisoned_constant_and_tiny_groups_on_the_device(dtype, bits):
    n = 64 * 2 + 37
    clean = values(n, dtype, 4)
    cases = {'clean': clean.clone()}
    for name, (at, value) in {'nan': (70, float('nan')), 'inf': (100, float('inf')), '-inf': (64, -float('inf'))}.items():
        cases[name] = clean.clone()
        cases[name][at] = value
    fi = torch.finfo(dtype)
    cases['overflow'] = clean.clone()
    cases['overflow'][64], cases['overflow'][127] = fi.max, -fi.max   # fp32 / bf16: the range is not finite; fp16: it is, and the group is clean
    cases['constant'] = clean.clone()
    cases['constant'][64:128] = 0.3
    cases['zeros'] = clean.clone()
    cases['zeros'][64:128] = 0.0
    cases['zeros'][64:128:3] = -0.0
    cases['tiny'] = clean.clone()                                     # denormal ranges (fp16: its own denormals, normal fp32 numbers)
    cases['tiny'][64:128] = (torch.arange(64) % 5).to(dtype) * fi.smallest_normal * fi.eps
    for name, x in cases.items():
        want = cabi_x.quant_pack_host(x.float(), SEED, bits)
        for offset in (0, 1):
            packed = cabi_x.quant_pack(placed(x, offset), SEED, bits)
            assert_bytes(packed, want, f'{dtype} bits {bits} {name} offset {offset}')
        decoded = cabi_x.quant_unpack(packed, n, bits, dtype)
        assert_values(decoded, cabi_x.quant_unpack_host(want, n, bits).to(dtype), f'{dtype} bits {bits} {name} decoded')
        poisoned = name in ('nan', 'inf', '-inf') or (name == 'overflow' and dtype != torch.float16)
        assert bool(torch.isnan(decoded[64:128]).all()) == poisoned and not bool(torch.isnan(decoded[:64]).any()) and not bool(torch.isnan(decoded[128:]).any())
        if name in ('constant', 'zeros'):
            assert torch.equal(decoded[64:128].cpu(), x[64:128] + 0.0)     # exact (a -0 decodes to +0)


# ---- 2. unpack -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('packed_dtype', DTYPES, ids=ids)
def test_unpack_equals_the_host_decode_rounded_once(packed_dtype, bits, n):
    """(the buffer of each source dtype into each of the three output dtypes: bf16-packed data into fp16 and fp32 among them)"""
    packed = host_pack(n, packed_dtype, bits)
    decoded = cabi_x.quant_unpack_host(packed, n, bits)
    pbuf, pd = guarded_bytes(packed.numel())
    pd.copy_(packed)
    for dtype in DTYPES:
        want = decoded.to(dtype)
        for offset in (0, 1):                                         # 16-byte stores; the element path of an unaligned destination
            if n > 4096 and offset and dtype != packed_dtype:
                continue
            what = f'{packed_dtype} -> {dtype} bits {bits} n {n} offset {offset}'
            obuf = torch.full((offset + n + 8, ), 123.0, dtype=dtype, device=DEV)
            out = obuf[offset:offset + n]
            got = cabi_x.quant_unpack(pd, n, bits, dtype, out=out)
            assert got is out
            assert_values(out, want, what)
            assert bool((obuf[:offset] == 123.0).all()) and bool((obuf[offset + n:] == 123.0).all()), f'{what}: written outside the {n} elements'
    assert_bytes(pd, packed, 'packed changed')
    assert bool((pbuf[:GUARD] == SENTINEL).all()) and bool((pbuf[GUARD + packed.numel():] == SENTINEL).all())
    fresh = cabi_x.quant_unpack(pd, n, bits, torch.float32)
    assert fresh.shape == (n, ) and fresh.dtype == torch.float32
    assert_values(fresh, decoded, 'allocated out')


@pytest.mark.parametrize('bits', BITS)
def test_round_trip_is_within_one_step(bits):
    n = 2573
    x = values(n, torch.float32, 6).to(DEV)
    packed = cabi_x.quant_pack(x, SEED, bits)
    step = packed[:8 * ((n + 63) // 64)].view(torch.float32)[1::2].repeat_interleave(64)[:n]
    err = (cabi_x.quant_unpack(packed, n, bits, torch.float32).double() - x.double()).abs()
    assert bool((err <= step.double() * (1 + 2.0**-20)).all())


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_raised_before_any_launch():
    n = 2573
    x = values(n, torch.bfloat16).to(DEV)
    need = cabi_x.quant_bytes(n, 4)
    buf, out = guarded_bytes(need)
    with pytest.raises(cabi.FewbitHipError, match='bits must be 2, 4 or 8'):
        cabi_x.quant_pack(x, SEED, 3, out=out)
    with pytest.raises(cabi.FewbitHipError, match=f'{need - 1} bytes, {need} are needed'):
        cabi_x.quant_pack(x, SEED, 4, out=out[:need - 1])
    with pytest.raises(cabi.FewbitHipError, match='contiguous'):
        cabi_x.quant_pack(x[::2], SEED, 4)
    with pytest.raises(cabi.FewbitHipError, match='at least'):
        cabi_x.quant_unpack(out[:need - 1], n, 4, torch.float32)
    with pytest.raises(cabi.FewbitHipError, match='bits must be 2, 4 or 8'):
        cabi_x.quant_unpack(out, n, 3, torch.float32)
    # the library itself, on real device pointers: bits 3, a short buffer, a misaligned seed word, a misaligned buffer
    L, stream = cabi_x.lib(), torch.cuda.current_stream().cuda_stream
    err = lambda: L.fewbit_hipx_last_error().decode()
    words = torch.zeros(2, dtype=torch.int64, device=DEV)
    bf16 = cabi.DTYPES[torch.bfloat16]
    assert L.fewbit_hipx_quant_pack(bf16, x.data_ptr(), n, 3, SEED, None, out.data_ptr(), need, stream) == -1 and 'bits = 3' in err()
    assert L.fewbit_hipx_quant_pack(bf16, x.data_ptr(), n, 4, SEED, None, out.data_ptr(), need - 1, stream) == -1 and 'are needed' in err()
    assert L.fewbit_hipx_quant_pack(bf16, x.data_ptr(), n, 4, SEED, words.data_ptr() + 4, out.data_ptr(), need, stream) == -1 and 'seed word' in err()
    assert L.fewbit_hipx_quant_pack(bf16, x.data_ptr(), n, 4, SEED, None, out.data_ptr() + 4, need, stream) == -1 and '8-byte aligned' in err()
    assert L.fewbit_hipx_quant_pack(bf16, x.data_ptr() + 1, n, 4, SEED, None, out.data_ptr(), need, stream) == -1 and 'aligned' in err()
    assert L.fewbit_hipx_quant_unpack(out.data_ptr(), n, 3, bf16, x.data_ptr(), stream) == -1 and 'bits = 3' in err()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()), 'a refused call wrote'     # nothing ran
    assert cabi_x.quant_pack(x[:0], SEED, 4).numel() == 0 and cabi_x.quant_unpack(out[:0], 0, 4, torch.float16).numel() == 0


# ---- 4. graph capture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bits', BITS)
def test_a_captured_pack_rounds_afresh_on_every_replay(bits):
    """the seed is a device word the kernel reads when it runs: each replay's buffer is the host evaluation of the word it read"""
    n, base = 2573, 0x7654321
    x = values(n, torch.bfloat16, 8)
    xd = x.to(DEV)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    word = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.zeros(cabi_x.quant_bytes(n, bits), dtype=torch.uint8, device=DEV)

    def step():
        cabi.next_sketch_seed(counter, base, out=word)
        cabi_x.quant_pack(xd, word, bits, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                        # an eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    c0 = int(counter)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    assert int(counter) == c0
    seen = []
    for replay in range(2):
        g.replay()
        torch.cuda.synchronize()
        seed = int(word) & 0xffffffffffffffff
        assert seed == cabi.mix_sketch_seed(base, c0 + replay)
        assert_bytes(out, cabi_x.quant_pack_host(x.float(), seed, bits), f'replay {replay}')
        seen.append(out.clone())
    assert not torch.equal(seen[0], seen[1])
