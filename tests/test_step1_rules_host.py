"""tests/step1_reference.py (the host restatement of the 1-bit family that tests/test_gpu_step1_exhaustive.py holds the kernels to) against
ATen's own forward and autograd on the host, for every bf16 and fp16 input: bit-identical in value and in gradient (gy = 1) on every finite
nonzero input.  Where the two differ is part of the contract and asserted as a set, per function: only NaN inputs and the two zeros, and of
those exactly the ones named in DIFFERS (a NaN result on both sides counts as equal: NaN payloads are not part of parity)."""
import pytest
import torch

import step1_reference as ref

CASES = [('hardshrink', (0.5, )), ('hardsigmoid', ()), ('hardtanh', (-1.0, 1.0)), ('leaky_relu', (0.5, )), ('leaky_relu', (0.01, )), ('relu', ()),
         ('relu6', ()), ('softshrink', (0.5, )), ('threshold', (1.0, 3.0))]

# name: (inputs whose VALUE differs from ATen's, inputs whose GRADIENT differs), each a set of 'nan' (every NaN pattern), '+0', '-0'.
#   hardshrink, softshrink   a NaN fails both comparisons of the reference's kernel and takes the zero branch; ATen returns the NaN
#   hardsigmoid, hardtanh,   a NaN is on neither clamped side, so the kernels' bit says "sloped piece" and the gradient is the multiplier;
#   relu6                    ATen's backward tests (x > lo) && (x < hi), false for NaN: gradient 0
#   relu, relu6              x <= 0 gives +0 for both zeros; ATen's clamp keeps -0
#   leaky_relu               x >= 0 is the identity side (gradient 1 at both zeros); ATen takes the slope unless x > 0
DIFFERS = {'hardshrink': ({'nan'}, set()), 'hardsigmoid': (set(), {'nan'}), 'hardtanh': (set(), {'nan'}), 'leaky_relu': (set(), {'+0', '-0'}),
           'relu': ({'-0'}, set()), 'relu6': ({'-0'}, {'nan'}), 'softshrink': ({'nan'}, set()), 'threshold': (set(), set())}


def all_16bit(dtype):
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)


def differing(a, b):
    """positions whose bits differ, two NaNs counting as equal"""
    return (a.view(torch.int16) != b.view(torch.int16)) & ~(torch.isnan(a) & torch.isnan(b))


def expected(x, classes):
    pattern = x.view(torch.int16)
    want = torch.zeros_like(pattern, dtype=torch.bool)
    if 'nan' in classes:
        want |= torch.isnan(x)
    if '+0' in classes:
        want |= pattern == 0
    if '-0' in classes:
        want |= pattern == -32768
    return want


@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float16))
@pytest.mark.parametrize('name,p', CASES)
def test_restatement_is_aten_except_at_nan_and_zero(name, p, dtype):
    x = all_16bit(dtype)
    assert int(torch.isnan(x).sum()) == (254 if dtype == torch.bfloat16 else 2046)
    y, bit = ref.rules(name, x, *p)
    gx = ref.backward(name, torch.ones_like(x), bit, *p[:1])
    y_aten, gx_aten = ref.aten(name, x, *p)
    assert y.dtype == dtype and gx.dtype == dtype
    value, grad = DIFFERS[name]
    dv, dg = differing(y, y_aten), differing(gx, gx_aten)
    special = torch.isnan(x) | (x == 0)
    assert not bool((dv & ~special).any()) and not bool((dg & ~special).any()), (name, x[dv & ~special][:8], x[dg & ~special][:8])
    assert torch.equal(dv, expected(x, value)), (name, 'value', int(dv.sum()), x[dv != expected(x, value)][:8])
    assert torch.equal(dg, expected(x, grad)), (name, 'gradient', int(dg.sum()), x[dg != expected(x, grad)][:8])


def test_unrepresentable_parameters_compare_in_fp32():
    """the parameters are float32(p), never rounded to the tensor's dtype: bf16(0.3) = 0.30078125 > float32(0.3) is kept by hardshrink 0.3
    and shrunk by softshrink 0.3 to a nonzero value, and the bf16 below it is not"""
    x = torch.tensor([0.30078125, 0.298828125, -0.30078125], dtype=torch.bfloat16)
    y, bit = ref.rules('hardshrink', x, 0.3)
    assert bit.tolist() == [True, False, True] and y.tolist() == [0.30078125, 0.0, -0.30078125]
    y, bit = ref.rules('softshrink', x, 0.3)
    assert bit.tolist() == [True, False, True]
    want = (torch.tensor(0.30078125) - torch.tensor(0.3)).to(torch.bfloat16)
    assert y[0] == want and y[2] == -want and y[1] == 0


def test_multipliers_and_packing():
    assert ref.multipliers('hardsigmoid') == (0.0, float(torch.tensor(1.0) / torch.tensor(6.0)))
    assert ref.multipliers('leaky_relu', 0.01) == (1.0, float(torch.tensor(0.01)))
    assert ref.multipliers('relu') == (0.0, 1.0)
    bit = torch.tensor([1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0], dtype=torch.bool)
    assert ref.pack_bits(bit).tolist() == [0x81, 0x03]
    gy = torch.tensor([-2.0, 3.0], dtype=torch.float16)
    gx = ref.backward('relu', gy, torch.tensor([False, True]))
    assert gx.tolist() == [0.0, 3.0] and bool(torch.signbit(gx[0]))            # 0 * negative stays -0
