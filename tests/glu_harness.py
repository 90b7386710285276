"""What the tests of the gated product share (tests/test_glu_host.py, test_gpu_glu.py, test_gpu_glu_layer.py): the packed form of a seed restated
in numpy with the rounding domain as a parameter (the Philox of tests/norm_harness.py), the float64 formulas of the definition, the two halves of
a state and their host decode, and the bounds of the comparisons with float64."""
import math

import numpy as np
import torch

from fewbit_amd import cabi_x
from norm_harness import M32, order_keys, philox

NAN_BITS = 0x7fc00000
GATE_DOMAIN, UP_DOMAIN = 7, 8
UNIT = {torch.float32: 2.0**-24, torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8}          # half an ulp, relative
TINY = {torch.float32: 2.0**-149, torch.float16: 2.0**-24, torch.bfloat16: 2.0**-133}        # the smallest subnormal
FAST_CLASS = 2.0**-20                                                                        # the fp32 error allowed to the evaluation of act


# ---- the definition restated in numpy --------------------------------------------------------------------------------------------------------
def uniforms(n, seed, domain):
    """U(i) for i < n: block q = i >> 3, counter (q low, q high, 0, domain), word (i & 7) >> 1, low half for even i, high half for odd i"""
    q = np.arange((n + 7) // 8, dtype=np.uint64)
    words = np.stack(philox(q & M32, q >> np.uint64(32), 0, domain, seed), axis=1)             # blocks x 4
    i = np.arange(n)
    word = words[i >> 3, (i & 7) >> 1]
    u = np.where(i & 1, word >> np.uint64(16), word & np.uint64(0xffff))
    return u.astype(np.float32) / np.float32(65536)


def restated(x, bits, seed, domain):
    """-> the packed bytes of the float32 array `x` rounded in `domain`, from the text of the header"""
    n, levels = x.size, np.float32(2**bits - 1)
    U = uniforms(n, seed, domain)
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
    for block in codes.reshape(-1, 8)[:(n + 7) // 8]:
        word = sum(int(c) << (bits * j) for j, c in enumerate(block))
        out += word.to_bytes(bits, 'little')
    return np.frombuffer(bytes(out), dtype=np.uint8)


def part_bytes(n, bits):
    """bytes of one half of a state: the packed form filled up to a multiple of 8"""
    return -(-(8 * math.ceil(n / 64) + bits * math.ceil(n / 8)) // 8) * 8


def halves(state, n, bits):
    """(the gate part, the up part, the zero bytes behind each) of a host state"""
    used, part = cabi_x.quant_bytes(n, bits), part_bytes(n, bits)
    assert state.numel() == 2 * part
    return state[:used], state[part:part + used], torch.cat((state[used:part], state[part + used:]))


def decoded(state, n, bits):
    """(g^, u^) of a host state, fp32"""
    part = part_bytes(n, bits)
    return cabi_x.quant_unpack_host(state[:part].contiguous(), n, bits), cabi_x.quant_unpack_host(state[part:].contiguous(), n, bits)


# ---- the formulas of the definition in float64 ----------------------------------------------------------------------------------------------------
def act64(g, activation):
    g = g.double()
    return g * torch.sigmoid(g) if activation == 'silu' else g * 0.5 * torch.special.erfc(-g * math.sqrt(0.5))


def slope64(g, activation):
    g = g.double()
    if activation == 'silu':
        s = torch.sigmoid(g)
        return s * (1 + g * (1 - s))
    return 0.5 * torch.special.erfc(-g * math.sqrt(0.5)) + g * torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)


def slope_terms64(g, activation):
    """the sum of the magnitudes of the terms the one-operation-per-step formula of act' adds: what its fp32 error is relative to.  silu:
    s + s |g| (1 - s); gelu: 0.5 + 0.5 |erf| + |g| phi (Phi itself is 0.5 (1 + erf), a sum that cancels for g < 0)"""
    g = g.double()
    if activation == 'silu':
        s = torch.sigmoid(g)
        return s * (1 + g.abs() * (1 - s))
    return 0.5 + 0.5 * torch.erf(g * math.sqrt(0.5)).abs() + g.abs() * torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)


def torch_act(g, activation):
    return torch.nn.functional.silu(g) if activation == 'silu' else torch.nn.functional.gelu(g)


def ulp_error(got, exact):
    """|got - exact| in units of the fp32 ulp of `exact` (float64 tensors holding fp32 results and the exact values)"""
    exact = exact.double()
    ulp = torch.ldexp(torch.ones_like(exact), torch.frexp(exact.abs().clamp_min(2.0**-126))[1] - 24)
    return (got.double() - exact).abs() / ulp
