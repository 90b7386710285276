"""What the tests of the gated product share (tests/test_glu_host.py, test_gpu_glu.py, test_gpu_glu_layer.py): the packed form of a seed restated
in numpy with the rounding domain as a parameter (the Philox of tests/norm_harness.py), the float64 formulas of the definition, the two halves of
a state and their host decode, and the bounds of the comparisons with float64; for tests/test_gpu_glu_values.py and tests/test_glu_values_host.py
the committed ups, a float64 -> 16-bit conversion that rounds once, and the comparison of a 16-bit result with float64 up to the format's overflow."""
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


# ---- every 16-bit gate against a committed set of ups (tests/test_gpu_glu_values.py, tests/test_glu_values_host.py) ---------------------------------
# 16-bit formats: (significand bits with the hidden one, the smallest normal exponent, the largest exponent)
FORMAT = {torch.float16: (11, -14, 15), torch.bfloat16: (8, -126, 127)}
INT16 = torch.int16

# The ups of the exhaustive forward: 24 columns (a multiple of 8: the vector path), each exactly representable in bf16 AND fp16.  +-1; odd mantissas
# of eight significant bits (every bit of a bf16 significand in use, among them all ones and one-above-a-power-of-two); powers of two and odd
# multiples at both ends; +-0; the last three are not finite.
# How large the largest may be follows from the definition, not from a kernel: y = round(act(g) * u) with act AN FP32 NUMBER held to 2^-20
# relative, 16 fp32 ulps.  Where act(g) lies among fp32's subnormals an ulp is 2^-149 whatever the value, and the product carries |u| 16 2^-149 of
# it.  The bound's absolute term, the smallest bf16 subnormal 2^-133, is half taken by the rounding of y itself (2^-134), so the other half
# absorbs the evaluation of act while |u| 2^-145 <= 2^-134: |u| <= 2^11.  (fp16 widens to normal fp32 numbers and needs no such limit: 2^11
# times its largest gates is far past its largest finite value.)  At the small end 2^-12 takes the whole lowest binades of both formats below
# their smallest subnormals.  With gates up to the largest finite value every |u| > 1 crosses the overflow threshold, every |u| < 1 the subnormals.
UPS = (1.0, -1.0, 0.0, -0.0, 1.0078125, -1.9921875, 1.3359375, -0.66796875, 3.0, 0.33203125, -1.6640625, 2048.0, -1536.0, 0.000244140625, -0.00042724609375,
       0.0107421875, 88.5, -0.0078125, 5.0, -0.1064453125, 0.7421875, float('nan'), float('inf'), float('-inf'))
FINITE_UPS = 21
# the ups of the exact-decode backward (rows of one gate and one up), four per gate over four calls, and the upstream gradients (by row)
BACK_UPS = (1.0, -1.9921875, 0.33203125, -1536.0, 1.3359375, -0.0078125, 88.5, -1.0)
BACK_GY = (1.0, -1.5, 0.7421875, -1.0078125, 1.9921875, -0.33203125, 2.5, -0.083984375, 0.5, -1.6640625, 1.1640625)


def round_once(x, dtype):
    """float64 -> bf16 / fp16, rounded ONCE to nearest, ties to even, with the format's subnormals and its overflow to infinity (torch converts
    float64 to either through fp32: two roundings).  The quotient by the quantum is exact (a power of two), torch.round is ties-to-even, and
    the rounded value is exact in fp32, so the last two conversions round nothing."""
    p, emin, emax = FORMAT[dtype]
    x = x.double()
    exponent = torch.frexp(x)[1] - 1                                                        # floor(log2 |x|); anything for 0, inf and NaN
    quantum = torch.ldexp(torch.ones_like(x), exponent.clamp(emin, emax) - (p - 1))
    r = torch.round(x / quantum) * quantum
    r = torch.where(r.abs() >= 2.0**(emax + 1), torch.copysign(torch.full_like(x, math.inf), x), r)
    r = torch.where(torch.isfinite(x), r, x)
    return r.float().to(dtype)


def finite_patterns(dtype):
    """every finite value of a 16-bit dtype (both zeros and the subnormals among them), by pattern 0x0000 .. 0xffff"""
    every = torch.arange(65536, dtype=torch.int32).to(INT16).view(dtype)
    return every[torch.isfinite(every.float())]


def zones(exact, dtype):
    """(bounded, band, beyond) of float64 results: |R| < max (1 - 2 h), where the bound applies and the result is finite; |R| > max (1 + 2 h),
    where the result is the infinity of R's sign; in between the largest finite value, that infinity, or a finite value within the bound is accepted.  Non-finite R: none of them."""
    top, h, a = float(torch.finfo(dtype).max), UNIT[dtype], exact.abs()
    finite = torch.isfinite(exact)
    bounded, beyond = finite & (a < top * (1 - 2 * h)), finite & (a > top * (1 + 2 * h))
    return bounded, finite & ~bounded & ~beyond, beyond


def held(got, exact, dtype, fp32_error_of=None, vanishing=None):
    """the comparison of a 16-bit result with float64, element by element -> (ok, half_ulps, band): the existing bound (UNIT, FAST_CLASS, TINY)
    on the bounded zone, where the result must be finite; the signed infinity beyond; either in the band; a zero of float64's sign where R
    is a zero; NaN exactly where R is one; R itself where R is infinite.
    `fp32_error_of`: what the 2^-20 is taken of (default |R|).  It is given for d_gate, whose act' is a SUM: there the sign of a zero is not
    held to float64's (at gelu's g = -38.5 both terms underflow in float64 and the sign of the zero is that of the one that gave way last).
    `vanishing`: where an infinite up met a finite gate whose act is below what fp32 can hold (`act_vanishes`): NaN or R is accepted.
    `half_ulps`: the error beyond the absolute terms in half ulps of R (0 outside the bounded zone and at R = 0)"""
    top = float(torch.finfo(dtype).max)
    g = got.double()
    bounded, band, beyond = zones(exact, dtype)
    absolute = TINY[dtype] + (0 if fp32_error_of is None else FAST_CLASS * fp32_error_of)
    relative = UNIT[dtype] + (FAST_CLASS if fp32_error_of is None else 0)
    error = (g - exact).abs()
    near = torch.isfinite(g) & (error <= relative * exact.abs() + absolute)
    infinity = g == torch.copysign(torch.full_like(g, math.inf), exact)
    ok = bounded & near
    ok |= beyond & infinity
    # (the band starts two ulps below the largest finite value: its lower part rounds to the value below the largest, which the bound admits)
    ok |= band & (infinity | (g == torch.copysign(torch.full_like(g, top), exact)) | near)
    ok |= torch.isnan(exact) & torch.isnan(g)
    ok |= torch.isinf(exact) & (g == exact)
    if fp32_error_of is None:
        ok &= ~((exact == 0) & ((g != 0) | (torch.signbit(g) != torch.signbit(exact))))
    if vanishing is not None:
        ok |= vanishing & torch.isnan(g)
    half_ulps = torch.where(bounded & (exact != 0), (error - absolute) / (UNIT[dtype] * exact.abs().clamp_min(1e-320)), torch.zeros_like(error))
    return ok, half_ulps, band


def act_vanishes(gate, up, activation):
    """where `up` is infinite and `gate` is finite with 0 < |act64(gate)| < 16 * 2^-149.  The definition evaluates act in fp32 to 16 ulps, an
    ulp among the subnormals is 2^-149, so there the fp32 act may be a zero and the product with the infinity a NaN, while float64, whose
    range ends elsewhere (silu: g = -745, gelu: g = -38.5), still has a signed infinity"""
    a = act64(gate, activation).abs()
    return torch.isinf(up.double()) & torch.isfinite(gate.double()) & (a > 0) & (a < 2.0**-145)


def one_ulp_off(got, exact, dtype):
    """how many finite results are the neighbour of the correctly rounded one"""
    want = round_once(exact, dtype)
    both = torch.isfinite(got.float()) & torch.isfinite(want.float())
    return int(((got.view(INT16).int() - want.view(INT16).int()).abs() == 1)[both].sum())


def gate_up_grid(dtype):
    """(gate, up) of the exhaustive forward, 65536 x 24: row r holds pattern r of the dtype, column c holds UPS[c]"""
    gate = torch.arange(65536, dtype=torch.int32).to(INT16).view(dtype)[:, None].expand(65536, len(UPS)).contiguous()
    up = torch.tensor(UPS, dtype=torch.float64).to(dtype)[None, :].expand(65536, len(UPS)).contiguous()
    return gate, up


def exact_product(gate, up, activation):
    """act64(gate) * up in float64: NaN for a NaN of either, for inf * 0 and for silu and gelu of -inf (-inf * 0, in the kernels as here)"""
    return act64(gate, activation) * up.double()


FP32_UPS = (1.0, -1.5, 3.0, 0.33203125, -0.000244140625, 88.5, 1.00000011920928955078125, -0.7853981852531433)


def fp32_gates():
    """helpers.probe_patterns with the +-1 and +-2 ulp neighbours of +-0.5, and the stretches where the 16-bit formulas change: -14.3 .. -14.2
    (erfc leaves the normal range) and +-87 .. +-105 (the sigmoid leaves it); a multiple of 8 of them (the first ones repeated)"""
    from helpers import probe_patterns
    tail = torch.linspace(87.0, 105.0, 577)
    g = torch.cat([probe_patterns(torch.float32, kinks=(0.5, -0.5)), torch.linspace(-14.3, -14.2, 257), tail, -tail])
    return torch.cat([g, g[:-g.numel() % 8]])


def ulp_error(got, exact):
    """|got - exact| in units of the fp32 ulp of `exact` (float64 tensors holding fp32 results and the exact values)"""
    exact = exact.double()
    ulp = torch.ldexp(torch.ones_like(exact), torch.frexp(exact.abs().clamp_min(2.0**-126))[1] - 24)
    return (got.double() - exact).abs() / ulp
