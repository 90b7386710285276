"""What tests/test_gpu_glu_values.py leans on, checked without a GPU: the float64 -> 16-bit helper that rounds ONCE, the committed inputs (on them
the correctly rounded float64 result alone breaks the bound nowhere, and the band around the largest finite value that the value check leaves
out is at most 0.1 % of the finite cases: the inputs were chosen for the reference, not for a kernel), and the PyTorch formulation of
``glu_quantized`` on groups that decode exactly, held to the same float64 formulas."""
import math

import pytest
import torch

import fewbit_amd as fewbit
from glu_harness import (BACK_GY, BACK_UPS, FAST_CLASS, FINITE_UPS, FORMAT, FP32_UPS, INT16, UNIT, UPS, act64, exact_product, finite_patterns, fp32_gates,
                         gate_up_grid, held, one_ulp_off, round_once, slope64, slope_terms64)

SIXTEEN = (torch.float16, torch.bfloat16)
ACTIVATIONS = ('silu', 'gelu')
ids = lambda d: str(d).split('.')[-1]


# ---- the helper --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', SIXTEEN, ids=ids)
def test_round_once_keeps_every_pattern_and_rounds_the_ties_between_neighbours_to_even(dtype):
    every = torch.arange(65536, dtype=torch.int32).to(INT16).view(dtype)
    kept = round_once(every.double(), dtype)
    number = ~torch.isnan(every.float())
    assert torch.equal(kept.view(INT16)[number], every.view(INT16)[number]) and bool(torch.isnan(kept.float()[~number]).all())
    # neighbours a < b of one sign by pattern (positive: 0x0000 .. 0x7bff / 0x7f7f, then the step to infinity), and their midpoint in float64
    top = int(torch.tensor(torch.finfo(dtype).max, dtype=dtype).view(INT16))
    low = torch.arange(0, top, dtype=torch.int32)
    a, b = low.to(INT16).view(dtype).double(), (low + 1).to(INT16).view(dtype).double()
    tie = (a + b) / 2                                                       # exact: one more bit than the format
    even = torch.where(low % 2 == 0, a, b)
    for sign in (1.0, -1.0):
        assert torch.equal(round_once(sign * tie, dtype).double(), sign * even)
        assert torch.equal(round_once(sign * torch.nextafter(tie, a), dtype).double(), sign * a)
        assert torch.equal(round_once(sign * torch.nextafter(tie, b), dtype).double(), sign * b)
    # beyond the largest finite value: its tie with 2^(emax + 1) goes to the even side, infinity
    p, emin, emax = FORMAT[dtype]
    largest = float(torch.finfo(dtype).max)
    edge = torch.tensor([(largest + 2.0**(emax + 1)) / 2], dtype=torch.float64)
    assert float(round_once(edge, dtype)) == math.inf and float(round_once(torch.nextafter(edge, torch.zeros(1, dtype=torch.float64)), dtype)) == largest
    assert float(round_once(-edge, dtype)) == -math.inf
    # half the smallest subnormal: a tie with zero, to zero, the sign kept; the numbers this side of it too
    tiny = torch.tensor([2.0**(emin - p + 1)], dtype=torch.float64)
    zero = round_once(-tiny / 2, dtype)
    assert float(zero) == 0 and bool(torch.signbit(zero)) and float(round_once(torch.nextafter(tiny / 2, tiny), dtype)) == float(tiny)
    nan_and_inf = round_once(torch.tensor([math.nan, math.inf, -math.inf], dtype=torch.float64), dtype).float()
    assert bool(torch.isnan(nan_and_inf[0])) and nan_and_inf[1:].tolist() == [math.inf, -math.inf]


def test_round_once_differs_from_the_conversion_through_fp32():
    """1 + 2^-8 + 2^-30 lies above the tie of bf16's 1 and 1 + 2^-7; fp32 rounds it to the tie, and the second rounding goes to even, down"""
    x = torch.tensor([1 + 2.0**-8 + 2.0**-30], dtype=torch.float64)
    assert float(round_once(x, torch.bfloat16)) == 1 + 2.0**-7 and float(x.float().to(torch.bfloat16)) == 1.0


# ---- the committed inputs ----------------------------------------------------------------------------------------------------------------------------
def test_the_ups_are_exact_in_both_formats_and_hold_what_the_cases_need():
    ups = torch.tensor(UPS, dtype=torch.float64)
    for dtype in SIXTEEN:
        back = ups.to(dtype).double()
        assert torch.equal(back[:FINITE_UPS], ups[:FINITE_UPS]) and torch.equal(torch.signbit(back), torch.signbit(ups))
    finite = ups[:FINITE_UPS]
    assert len(UPS) % 8 == 0 and FINITE_UPS >= 16 and bool(torch.isfinite(finite).all()) and not bool(torch.isfinite(ups[FINITE_UPS:]).any())
    assert 1.0 in UPS and -1.0 in UPS and sum(1 for u in UPS if u == 0 and math.copysign(1, u) > 0) == 1 and sum(1 for u in UPS if u == 0 and math.copysign(1, u) < 0) == 1
    mantissa = torch.frexp(finite[finite != 0])[0].abs() * 256                         # eight significant bits: an odd integer uses them all
    assert int((mantissa % 2 == 1).sum()) >= 4
    assert float(finite.abs().max()) == 2.0**11 and float(finite[finite != 0].abs().min()) == 2.0**-12
    assert set(BACK_UPS) <= set(UPS) and len(set(BACK_UPS)) >= 4 and len({math.copysign(1, v) for v in BACK_GY}) == 2
    for dtype in SIXTEEN:
        assert torch.equal(torch.tensor(BACK_GY, dtype=torch.float64).to(dtype).double(), torch.tensor(BACK_GY, dtype=torch.float64))


@pytest.mark.parametrize('activation', ACTIVATIONS)
@pytest.mark.parametrize('dtype', SIXTEEN, ids=ids)
def test_the_correctly_rounded_reference_breaks_the_bound_nowhere_and_the_band_is_small(dtype, activation):
    gate, up = gate_up_grid(dtype)
    exact = exact_product(gate, up, activation)
    ok, half_ulps, band = held(round_once(exact, dtype), exact, dtype)
    finite = torch.isfinite(gate.float()) & torch.isfinite(up.float())
    assert int(finite.sum()) == finite_patterns(dtype).numel() * FINITE_UPS
    assert int((~ok).sum()) == 0, (gate[~ok][:4], up[~ok][:4])
    assert float(half_ulps.max()) <= 1.0
    assert float(band.sum()) / float(finite.sum()) <= 0.001
    assert one_ulp_off(round_once(exact, dtype)[finite], exact[finite], dtype) == 0
    # the backward's rows: d_up, the product and d_gate of the reference, every gate against the four ups it meets
    gates = finite_patterns(dtype)
    r = torch.arange(gates.numel())
    for call in range(4):
        ups = torch.tensor(BACK_UPS, dtype=torch.float64)[(r + call) % len(BACK_UPS)]
        gys = torch.tensor(BACK_GY, dtype=torch.float64)[(3 * r + call) % len(BACK_GY)]
        act, pair = act64(gates.double() + 0.0, activation), gys * ups
        for exact, scale in ((gys * act, None), (act * ups, None), (pair * slope64(gates, activation), pair.abs() * slope_terms64(gates, activation))):
            ok, _, band = held(round_once(exact, dtype), exact, dtype, scale)
            assert bool(ok.all()) and float(band.sum()) / gates.numel() <= 0.001


# ---- the PyTorch formulation on groups that decode exactly ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('activation', ACTIVATIONS)
def test_the_pytorch_formulation_on_constant_groups_at_the_fp32_probe_gates(activation):
    """host tensors: rows of 64 times one gate and one up decode to themselves (step 0, every code 0; -0 to +0), so the formulation's gradients
    are ``gy * act(g)`` and ``gy * u * act'(g)`` on known inputs.  Both are torch's own fp32 formulas: act is accurate to fp32 relative to |g|, not
    to act(g) (ATen's gelu cancels in 1 + erf, its silu is 0 where exp(-g) has overflowed), so d_up is held to half an ulp of R plus 2^-20 of
    |gy g|; d_gate to half an ulp plus 2^-20 of the magnitudes of its terms, as on the kernels."""
    g = fp32_gates()
    g = g[torch.isfinite(g)]
    rows = g.numel()
    r = torch.arange(rows)
    ups, gys = torch.tensor(FP32_UPS)[r % len(FP32_UPS)], torch.tensor(BACK_GY)[(3 * r) % len(BACK_GY)]
    wide = lambda v: v[:, None].expand(rows, 64).contiguous()
    gate, up = wide(g).requires_grad_(), wide(ups).requires_grad_()
    y = fewbit.functional.glu_quantized(gate, up, activation, 4, torch.Generator().manual_seed(5))
    d_gate, d_up = torch.autograd.grad(y, (gate, up), wide(gys))
    for t in (d_gate, d_up):
        assert bool((t.view(torch.int32) == t.view(torch.int32)[:, :1]).all())
    g_hat, pair = g.double() + 0.0, gys.double() * ups.double()
    scale = UNIT[torch.float32] + FAST_CLASS
    tame = torch.isfinite(pair * g_hat) & (g_hat.abs() < 1e30)                                     # (gy u g finite in fp32 with room to spare)
    want_up = gys.double() * act64(g_hat, activation)
    assert bool(((d_up[:, 0].double() - want_up).abs() <= scale * (gys.double() * g_hat).abs() + 2.0**-149)[tame].all())
    want_gate, terms = pair * slope64(g_hat, activation), pair.abs() * slope_terms64(g_hat, activation)
    # (torch's fp32 sigmoid is 1 / (1 + exp(-g)): 0 once exp(-g) has overflowed, where the true s is below 2^-128; s (1 + g (1 - s)) loses that)
    lost = pair.abs() * (1 + g_hat.abs()) * 2.0**-128
    error = (d_gate[:, 0].double() - want_gate).abs()
    ok = error <= UNIT[torch.float32] * want_gate.abs() + FAST_CLASS * terms + lost + 2.0**-149
    assert bool(ok[tame].all()), (g[tame][~ok[tame]][:8], float((error / terms.clamp_min(1e-300))[tame].max()))
