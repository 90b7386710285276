"""The packed form of a seed without a GPU (include/fewbit_hipx.h; fewbit_amd/csrc/fewbit_quant.hip): the five entry points of the companion
library (declared, exported, bound), the host evaluation against an independent numpy restatement of the header's definition (Philox in
numpy, checked against the frozen library's), the size formula, the decode bound, unbiasedness over 4000 seeds, poisoned groups, the padding
bits, the refusals before anything is launched, and ``fewbit.QuantizedLinear`` on host tensors."""
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fewbit_amd as fewbit
from fewbit_amd import cabi, cabi_x, linear
from norm_harness import M32, order_keys, philox, saved_by

ROOT = Path(__file__).resolve().parents[1]
QUANT_SYMBOLS = ('fewbit_hipx_quant_bytes', 'fewbit_hipx_quant_pack_host', 'fewbit_hipx_quant_unpack_host', 'fewbit_hipx_quant_pack',
                 'fewbit_hipx_quant_unpack')
BITS = (2, 4, 8)
SIZES = (1, 7, 8, 9, 63, 64, 65, 205, 2573)
SEED = 0x1234567887654321
NAN_BITS = 0x7fc00000


# ---- the definition restated in numpy ----------------------------------------------------------------------------------------------------
def uniforms(n, seed):
    """U(i) for i < n: block q = i >> 3, counter (q low, q high, 0, 7), word (i & 7) >> 1, low half for even i, high half for odd i"""
    q = np.arange((n + 7) // 8, dtype=np.uint64)
    words = np.stack(philox(q & M32, q >> np.uint64(32), 0, 7, seed), axis=1)                  # blocks x 4
    i = np.arange(n)
    word = words[i >> 3, (i & 7) >> 1]
    u = np.where(i & 1, word >> np.uint64(16), word & np.uint64(0xffff))
    return u.astype(np.float32) / np.float32(65536)


def restated(x, bits, seed):
    """-> the packed bytes of the float32 array `x`, from the text of the header"""
    n, levels = x.size, np.float32(2**bits - 1)
    U = uniforms(n, seed)
    params, codes = [], np.zeros(8 * ((n + 7) // 8), dtype=np.uint64)
    with np.errstate(all='ignore'):
        for first in range(0, n, 64):
            xs = x[first:first + 64]
            keys = order_keys(xs)
            lo, hi = xs[np.argmin(keys)], xs[np.argmax(keys)]
            span = np.float32(hi - lo)
            if not np.isfinite(xs).all() or not np.isfinite(span):
                params += [NAN_BITS, NAN_BITS]
                continue
            step = np.float32(span / levels)
            inv = np.float32(levels / span) if span > 0 else np.float32(0)
            if not np.isfinite(inv):
                inv = np.float32(0)
            t = ((xs - lo).astype(np.float32) * inv).astype(np.float32)
            s = (t + U[first:first + 64]).astype(np.float32)
            codes[first:first + xs.size] = np.minimum(np.floor(s), levels).astype(np.uint64)
            params += [int(np.array(lo).view(np.uint32)), int(np.array(step).view(np.uint32))]
    out = bytearray(np.array(params, dtype='<u4').tobytes())
    for block in codes.reshape(-1, 8):
        word = sum(int(c) << (bits * j) for j, c in enumerate(block))
        out += word.to_bytes(bits, 'little')
    return np.frombuffer(bytes(out), dtype=np.uint8)


def draw(n, kind, salt=0):
    g = torch.Generator().manual_seed(77 + salt)
    if kind == 'normal':
        return torch.randn(n, generator=g)
    if kind == 'narrow':
        return 1.0 + 1e-3 * torch.randn(n, generator=g)
    if kind == 'constant':
        return torch.full((n, ), 0.3)
    if kind == 'zeros':                                              # -0 and +0 in one group: lo = -0, hi = +0, range +0
        x = torch.zeros(n)
        x[::3] = -0.0
        return x
    if kind == 'tiny':                                               # ranges around and below L / FLT_MAX, denormals included
        return torch.randn(n, generator=g) * torch.tensor([1e-36, 1e-38, 1e-41, 3e-45]).repeat(n // 4 + 1)[:n].repeat_interleave(1)
    raise KeyError(kind)


def steps_of(packed, n):
    """the step of every element's group, as float32"""
    groups = (n + 63) // 64
    return packed[:8 * groups].view(torch.float32)[1::2].repeat_interleave(64)[:n]


# ---- the library: symbols, sizes, the definition ------------------------------------------------------------------------------------------
def test_the_five_symbols_are_exported_declared_and_bound():
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    declared = set(re.findall(r'\b(fewbit_hipx_\w+)\s*\(', header))
    out = subprocess.run(['nm', '-D', '--defined-only', str(cabi_x.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in QUANT_SYMBOLS:
        assert name in declared and name in exported and name in cabi_x.SYMBOLS, name
    assert cabi_x.lib().fewbit_hipx_revision() == cabi_x.REVISION == 2
    assert 'fewbit_hipx_quant_bytes, _quant_pack_host, _quant_unpack_host, _quant_pack, _quant_unpack' in header


def test_the_numpy_philox_is_the_frozen_librarys():
    for counter, seed in (((0, 0, 0, 0), 0), ((5, 1, 0, 7), SEED), ((0xffffffff, 0xffffffff, 0, 7), 2**64 - 1)):
        got = tuple(int(w) for w in philox(*counter, seed))
        assert got == cabi.philox4x32(counter, (seed & 0xffffffff, seed >> 32)), counter
    assert tuple(int(w) for w in philox(0, 0, 0, 0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)


def test_quant_bytes_is_the_formula():
    for bits in BITS:
        for n in SIZES + (2**22, 2**36):
            assert cabi_x.quant_bytes(n, bits) == 8 * math.ceil(n / 64) + bits * math.ceil(n / 8), (n, bits)
        assert cabi_x.quant_bytes(0, bits) == 0 and cabi_x.quant_bytes(2**36 + 1, bits) == 0 and cabi_x.quant_bytes(-1, bits) == 0
    for bits in (0, 1, 3, 5, 16):
        assert cabi_x.quant_bytes(64, bits) == 0, bits
    # relative to a bf16 input: the table of the documents
    n = 2**20
    assert [cabi_x.quant_bytes(n, b) / (2 * n) for b in BITS] == [0.1875, 0.3125, 0.5625]


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('bits', BITS)
def test_pack_host_equals_the_definition_restated(bits, n):
    for kind in ('normal', 'narrow', 'constant', 'zeros', 'tiny'):
        x = draw(n, kind, n)
        for seed in (SEED, 7):
            got = cabi_x.quant_pack_host(x, seed, bits)
            assert got.numel() == cabi_x.quant_bytes(n, bits)
            want = restated(x.numpy(), bits, seed)
            assert np.array_equal(got.numpy(), want), (kind, seed, np.flatnonzero(got.numpy() != want)[:8])
    assert not torch.equal(cabi_x.quant_pack_host(draw(n, 'normal'), 1, bits), cabi_x.quant_pack_host(draw(n, 'normal'), 2, bits)) or n < 8


def test_u_uses_its_own_counter_word_and_carries_into_the_second():
    """(the dropout's u with counter word 3 = 7 in place of 5; block 2^32 has counter word 1 = 1 -- only the numpy side is evaluated there)"""
    u5 = np.stack(philox(np.arange(4), 0, 0, 5, SEED), axis=1)
    u7 = np.stack(philox(np.arange(4), 0, 0, 7, SEED), axis=1)
    assert not np.array_equal(u5, u7)
    U = uniforms(64, SEED)
    assert U.dtype == np.float32 and (U >= 0).all() and (U < 1).all() and np.array_equal(U * 65536, np.round(U * 65536))


# ---- the decode ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('kind', ('normal', 'narrow', 'constant'))
def test_decode_is_within_one_step_of_every_element(kind, bits):
    for n in (205, 2573):
        x = draw(n, kind)
        packed = cabi_x.quant_pack_host(x, SEED, bits)
        decoded = cabi_x.quant_unpack_host(packed, n, bits)
        step = steps_of(packed, n)
        err = (decoded.double() - x.double()).abs()
        print(f'{kind} bits {bits} n {n}: max |error| / step = {float((err / step.double().clamp_min(1e-300)).max()):.6f}')
        assert bool((err <= step.double() * (1 + 2.0**-20)).all())
        if kind == 'constant':
            assert torch.equal(decoded, x) and bool((step == 0).all())


@pytest.mark.parametrize('bits', BITS)
def test_the_rounding_is_unbiased_over_4000_seeds(bits):
    """|mean(decode) - x| <= 5 step / (2 sqrt(4000)) on every element: step / 2 bounds the deviation of one draw"""
    n, seeds = 2573, 4000
    x = draw(n, 'normal', 5)
    total = torch.zeros(n, dtype=torch.float64)
    for seed in range(seeds):
        packed = cabi_x.quant_pack_host(x, 0xABCDEF0000 + seed, bits)
        total += cabi_x.quant_unpack_host(packed, n, bits).double()
    unit = steps_of(packed, n).double() / (2 * math.sqrt(seeds))
    worst = float(((total / seeds - x.double()).abs() / unit).max())
    print(f'bits {bits}: the worst element is {worst:.2f} units of step / (2 sqrt(seeds)) off')
    assert worst <= 5.0


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('poison', ('nan', 'inf', 'overflow'))
def test_a_poisoned_group_decodes_to_nan_and_touches_no_other(poison, bits):
    n = 64 * 2 + 37                                                  # three groups, the last ragged
    clean = draw(n, 'normal', 9)
    x = clean.clone()
    if poison == 'nan':
        x[70] = float('nan')
    elif poison == 'inf':
        x[100] = float('inf')
    else:
        x[64], x[127] = 3e38, -3e38                                  # both finite, their difference is not
    got, base = cabi_x.quant_pack_host(x, SEED, bits), cabi_x.quant_pack_host(clean, SEED, bits)
    decoded, decoded_clean = cabi_x.quant_unpack_host(got, n, bits), cabi_x.quant_unpack_host(base, n, bits)
    assert bool(torch.isnan(decoded[64:128]).all()) and torch.equal(decoded[:64], decoded_clean[:64]) and torch.equal(decoded[128:], decoded_clean[128:])
    assert decoded[64:128].view(torch.int32).tolist() == [NAN_BITS] * 64
    assert got[8:16].view(torch.int32).tolist() == [NAN_BITS, NAN_BITS]
    codes = 24                                                       # 8 bytes per group
    assert not bool(got[codes + 8 * bits:codes + 16 * bits].any())  # the codes of group 1 are 0
    same = torch.ones(got.numel(), dtype=torch.bool)
    same[8:16] = False
    same[codes + 8 * bits:codes + 16 * bits] = False
    assert torch.equal(got[same], base[same])
    assert np.array_equal(got.numpy(), restated(x.numpy(), bits, SEED))


@pytest.mark.parametrize('bits', BITS)
def test_the_padding_bits_of_the_last_word_are_zero(bits):
    for n in (1, 7, 9, 63, 65, 205, 2573):
        x = torch.linspace(-1, 1, 64).repeat(n // 64 + 1)[:n].flip(0)
        packed = cabi_x.quant_pack_host(x, SEED, bits)
        word = int.from_bytes(bytes(packed[-bits:].tolist()), 'little')
        assert word >> (bits * (n % 8)) == 0, n
        assert bool(packed[8 * math.ceil(n / 64):].any()) or n == 1


def test_calls_are_refused_by_code_and_text_before_anything_is_launched():
    """(null and fake pointers throughout: a call that got as far as a launch would fail loudly)"""
    L = cabi_x.lib()
    err = lambda: L.fewbit_hipx_last_error().decode()
    pack, unpack = L.fewbit_hipx_quant_pack, L.fewbit_hipx_quant_unpack
    fake = 4096                                                       # an aligned non-null address that is never dereferenced
    assert pack(3, fake, 64, 4, 1, None, fake, 1024, None) == -1 and 'dtype 3' in err()
    for bits in (0, 1, 3, 5, 16):
        assert pack(0, fake, 64, bits, 1, None, fake, 1024, None) == -1 and f'bits = {bits}' in err()
        assert unpack(fake, 64, bits, 0, fake, None) == -1 and f'bits = {bits}' in err()
    assert pack(0, None, 64, 4, 1, None, fake, 1024, None) == -1 and 'null' in err()
    assert pack(0, fake, 64, 4, 1, None, None, 1024, None) == -1 and 'null' in err()
    assert pack(0, fake + 2, 64, 4, 1, None, fake, 1024, None) == -1 and 'aligned' in err()
    assert pack(2, fake + 1, 64, 4, 1, None, fake, 1024, None) == -1 and 'aligned' in err()
    assert pack(2, fake, 64, 4, 1, None, fake + 4, 1024, None) == -1 and '8-byte aligned' in err()
    assert pack(2, fake, 64, 4, 1, None, fake, 39, None) == -1 and '39 bytes, 40 are needed' in err()
    assert pack(2, fake, 64, 4, 1, fake + 4, fake, 1024, None) == -1 and 'seed word' in err()
    assert pack(2, fake, 2**36 + 1, 4, 1, None, fake, 2**40, None) == -1 and '2^36' in err()
    assert unpack(fake, 64, 4, 5, fake, None) == -1 and 'dtype 5' in err()
    assert unpack(None, 64, 4, 0, fake, None) == -1 and 'null' in err()
    assert unpack(fake + 4, 64, 4, 0, fake, None) == -1 and '8-byte aligned' in err()
    assert unpack(fake, 64, 4, 0, fake + 2, None) == -1 and 'aligned' in err()
    # n = 0: nothing to do, whatever the pointers
    assert pack(0, None, 0, 4, 1, None, None, 0, None) == 0 and unpack(None, 0, 8, 1, None, None) == 0
    # the host functions
    assert L.fewbit_hipx_quant_pack_host(None, 8, 4, 1, fake) == -1 and 'null' in err()
    assert L.fewbit_hipx_quant_pack_host(fake, 8, 3, 1, fake) == -1 and 'bits = 3' in err()
    assert L.fewbit_hipx_quant_unpack_host(fake, 8, 4, None) == -1 and 'null' in err()
    assert L.fewbit_hipx_quant_pack_host(None, 0, 4, 1, None) == 0


def test_the_binding_refuses_host_tensors_and_unknown_widths():
    with pytest.raises(cabi.FewbitHipError, match='GPU'):
        cabi_x.quant_pack(torch.zeros(8), 1, 4)
    with pytest.raises(cabi.FewbitHipError, match='GPU'):
        cabi_x.quant_unpack(torch.zeros(16, dtype=torch.uint8), 8, 4, torch.float32)
    for call in (lambda: cabi_x.quant_pack_host(torch.zeros(8), 1, 3), lambda: cabi_x.quant_unpack_host(torch.zeros(64, dtype=torch.uint8), 8, 3)):
        with pytest.raises(cabi.FewbitHipError, match='bits must be 2, 4 or 8'):
            call()
    with pytest.raises(cabi.FewbitHipError, match='at least 12 bytes'):
        cabi_x.quant_unpack_host(torch.zeros(11, dtype=torch.uint8), 8, 4)
    assert cabi_x.quant_pack_host(torch.zeros(0), 1, 4).numel() == 0 and cabi_x.quant_unpack_host(torch.zeros(0, dtype=torch.uint8), 0, 4).numel() == 0


# ---- fewbit.QuantizedLinear on the host ----------------------------------------------------------------------------------------------------
ROWS, IN, OUT = 96, 24, 16


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('dtype', (torch.float32, torch.float64), ids=('float32', 'float64'))
def test_layer_on_host_tensors(dtype, bits):
    torch.manual_seed(3)
    layer = fewbit.QuantizedLinear(IN, OUT, dtype=dtype, bits=bits)
    x = torch.randn(4, ROWS // 4, IN, dtype=dtype, requires_grad=True)       # (three dimensions: the rows are the leading two)
    gy = torch.randn(4, ROWS // 4, OUT, dtype=dtype)
    xr = x.detach().clone().requires_grad_()
    yr = F.linear(xr, layer.weight, layer.bias)
    gxr, gwr, gbr = torch.autograd.grad(yr, (xr, layer.weight, layer.bias), gy)
    y, saved = saved_by(lambda: layer(x))
    assert type(y.grad_fn).__name__ == '_LinearQuantizedBackward' and torch.equal(y, yr)
    # what is kept: codes (one per byte), lo and step of every group, the weight -- nothing of the input's shape or size in a float dtype
    assert not any(t.shape == x.shape or t.shape == (ROWS, IN) for t in saved)
    assert not any(t.is_floating_point() and t.numel() >= x.numel() for t in saved)
    assert sorted(t.numel() for t in saved if t.dtype == torch.uint8) == [ROWS * IN]
    total, squares, calls = torch.zeros(OUT, IN, dtype=torch.float64), torch.zeros(OUT, IN, dtype=torch.float64), 400
    for _ in range(calls):
        gx, gw, gb = torch.autograd.grad(layer(x), (x, layer.weight, layer.bias), gy)
        assert torch.equal(gx, gxr) and torch.equal(gb, gbr)
        total += gw.double()
        squares += gw.double()**2
    mean = total / calls
    sd = (squares / calls - mean**2).clamp_min(0).sqrt() * math.sqrt(calls / (calls - 1))
    z = (mean - gwr.double()).abs() / (sd / math.sqrt(calls))
    print(f'{dtype} bits {bits}: worst entry {float(z.max()):.2f} standard errors; relative error of one call '
          f'{float((gw - gwr).norm() / gwr.norm()):.4f}')
    assert bool((sd > 0).all()) and float(z.max()) <= 5.0


def test_a_bf16_gradient_at_8_bits_is_not_biased_by_its_decode():
    """At 8 bits the step is about one bf16 ulp: X^ rounded to bf16 put the mean weight gradient of 200 calls 6 - 9 standard errors from the
    exact one (``linear._decode_in_two_terms``); the bound is that of the other widths and dtypes."""
    g = torch.Generator().manual_seed(31)
    x = torch.randn(256, 64, generator=g).bfloat16().requires_grad_()
    w = (torch.randn(32, 64, generator=g) / 8).bfloat16().requires_grad_()
    gy = torch.randn(256, 32, generator=g).bfloat16()
    exact = gy.double().T @ x.detach().double()
    torch.manual_seed(0)
    total, squares, calls = torch.zeros_like(exact), torch.zeros_like(exact), 200
    for _ in range(calls):
        (gw, ) = torch.autograd.grad(fewbit.functional.linear_quantized(x, w, None, 8), w, gy)
        assert gw.dtype == torch.bfloat16
        total += gw.double()
        squares += gw.double()**2
    mean = total / calls
    sd = (squares / calls - mean**2).clamp_min(0).sqrt() * math.sqrt(calls / (calls - 1))
    z = (mean - exact).abs() / (sd / math.sqrt(calls))
    print(f'bf16 at 8 bits on the host: worst entry {float(z.max()):.2f} standard errors')
    assert float(z.max()) <= 5.0


def test_layer_arguments_repr_and_exports():
    for bits in (0, 1, 3, 5, 16):
        with pytest.raises(ValueError, match='bits should be 2, 4 or 8'):
            fewbit.QuantizedLinear(4, 4, bits=bits)
        with pytest.raises(ValueError, match='bits should be 2, 4 or 8'):
            fewbit.functional.linear_quantized(torch.zeros(2, 4), torch.zeros(4, 4), None, bits=bits)
    m = fewbit.QuantizedLinear(4, 6, bias=False, bits=8)
    assert isinstance(m, torch.nn.Linear) and repr(m) == 'QuantizedLinear(in_features=4, out_features=6, bias=False, bits=8)'
    assert fewbit.QuantizedLinear(4, 6).bits == 4 and fewbit.QuantizedLinear(4, 6).generator is None
    assert fewbit.QuantizedLinear is linear.QuantizedLinear and fewbit.functional.linear_quantized is linear.linear_quantized
    assert {'QuantizedLinear', 'linear_quantized'} <= set(linear.__all__) and 'QuantizedLinear' not in fewbit.modules.__all__
    # map_module swaps the linears of a built model; the parameters are shared
    model = torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.GELU(), torch.nn.Sequential(torch.nn.Linear(8, 2, bias=False)), fewbit.LinearCRS(2, 2))
    weights = [model[0].weight, model[2][0].weight]
    model = fewbit.map_module(model, lambda m, path: fewbit.QuantizedLinear.from_linear(m, bits=2) if type(m) is torch.nn.Linear else m)
    swapped = [m for m in model.modules() if type(m) is fewbit.QuantizedLinear]
    assert [m.bits for m in swapped] == [2, 2] and [m.weight for m in swapped] == weights and swapped[1].bias is None
    assert type(model[3]) is fewbit.LinearCRS and model(torch.randn(5, 4)).shape == (5, 2)


def test_no_grad_and_a_frozen_weight_save_nothing_of_the_input():
    layer = fewbit.QuantizedLinear(IN, OUT)
    x = torch.randn(ROWS, IN, requires_grad=True)
    state = torch.get_rng_state()
    with torch.no_grad():
        y, saved = saved_by(lambda: layer(x))
    assert y.grad_fn is None and not saved and torch.equal(y, F.linear(x, layer.weight, layer.bias))
    layer.weight.requires_grad_(False)
    y, saved = saved_by(lambda: layer(x))
    assert 'Quantized' not in type(y.grad_fn).__name__ and not any(t.dtype == torch.uint8 for t in saved)
    assert not any(t.shape == x.shape for t in saved)
    y, saved = saved_by(lambda: layer(x[:0]))                         # no rows
    assert 'Quantized' not in type(y.grad_fn).__name__
    assert torch.equal(torch.get_rng_state(), state)                 # and nothing was drawn


def test_the_generator_decides_the_rounding_and_checkpointing_reproduces_it():
    from torch.utils.checkpoint import checkpoint
    x, w = torch.randn(ROWS, IN, requires_grad=True), torch.randn(OUT, IN, requires_grad=True)
    gy = torch.randn(ROWS, OUT)

    def grad_weight(generator=None):
        return torch.autograd.grad(fewbit.functional.linear_quantized(x, w, None, 2, generator), w, gy)[0]

    a, b = grad_weight(torch.Generator().manual_seed(4)), grad_weight(torch.Generator().manual_seed(4))
    assert torch.equal(a, b) and not torch.equal(a, grad_weight(torch.Generator().manual_seed(5)))
    torch.manual_seed(8)
    plain = grad_weight()
    for reentrant in (False, True):
        torch.manual_seed(8)
        y = checkpoint(lambda t, weight: fewbit.functional.linear_quantized(t, weight, None, 2), x, w, use_reentrant=reentrant)
        w.grad = None
        y.backward(gy)                                                # (re-entrant checkpointing takes backward(), not autograd.grad)
        assert torch.equal(w.grad, plain), reentrant
