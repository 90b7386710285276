"""Host restatement of the 1-bit family (stepwise1_*_kernel): value, derivative-branch bit and gradient multipliers of the eight
piecewise-linear activations, in plain torch on the host.  Test infrastructure (the checker), never the product path.

Where the rules come from: the bit rules and the multipliers are those of include/fewbit_hip.h and of the reference's kernels
(fewbit/cuda/codec.cu:298-487: which comparison is strict, which branch sets the bit); the value of each branch is ATen's formula
(hardsigmoid: (x + 3) / 6, relu6's upper branch: 6).  This file is NOT a translation of oracle/fewbit_oracle.c: it exists so that the
kernels are compared with something the oracle did not write.

Arithmetic: every comparison and every value is computed in fp32 on the fp32 image of the input, with the parameters as float32(p)
(never rounded to the tensor's dtype: a 16-bit tensor compares against float32(0.3), not against bf16(0.3)); the result is rounded ONCE
to the tensor's dtype.  The gradient is fp32(multiplier) * fp32(gy), rounded once.

    rules(name, x, p0, p1)        -> (y, bit): y in the dtype of x, bit a bool tensor
    multipliers(name, p0)         -> (m0, m1): the gradient multiplier of bit 0 / bit 1, python floats that float32 holds exactly
    backward(name, gy, bit, p0)   -> gx in the dtype of gy
    pack_bits(bit)                -> the packed state, uint8, bit i of byte i // 8 (LSB first), zero padded
    aten(name, x, p0, p1)         -> (y, grad for gy = 1) of torch.nn.functional on the host
"""
import torch
import torch.nn.functional as F

NAMES = ('hardshrink', 'hardsigmoid', 'hardtanh', 'leaky_relu', 'relu', 'relu6', 'softshrink', 'threshold')


def _f32(p: float) -> torch.Tensor:
    return torch.tensor(p, dtype=torch.float32)


def rules(name: str, x: torch.Tensor, p0: float = 0.0, p1: float = 0.0):
    xf = x.detach().cpu().float()
    a, b = _f32(p0), _f32(p1)
    zero = torch.zeros((), dtype=torch.float32)
    if name == 'hardshrink':                    # bit = kept; |x| <= lambda (and NaN: neither comparison holds) -> 0
        bit = (xf < -a) | (xf > a)
        y = torch.where(bit, xf, zero)
    elif name == 'hardsigmoid':                 # bit = the sloped middle piece
        lo, hi = xf <= -3.0, xf >= 3.0
        bit = ~(lo | hi)
        y = torch.where(lo, zero, torch.where(hi, _f32(1.0), (xf + 3.0) / 6.0))
    elif name == 'hardtanh':
        lo, hi = xf <= a, xf >= b
        bit = ~(lo | hi)
        y = torch.where(lo, a, torch.where(hi, b, xf))
    elif name == 'leaky_relu':                  # bit = the slope side; x >= 0 (both zeros) is the identity side
        pos = xf >= 0.0
        bit = ~pos
        y = torch.where(pos, xf, a * xf)
    elif name == 'relu':                        # x <= 0 (both zeros) -> +0
        off = xf <= 0.0
        bit = ~off
        y = torch.where(off, zero, xf)
    elif name == 'relu6':
        lo, hi = xf <= 0.0, xf >= 6.0
        bit = ~(lo | hi)
        y = torch.where(lo, zero, torch.where(hi, _f32(6.0), xf))
    elif name == 'softshrink':
        lo, hi = xf < -a, xf > a
        bit = lo | hi
        y = torch.where(lo, xf + a, torch.where(hi, xf - a, zero))
    elif name == 'threshold':                   # p0 = threshold, p1 = value
        off = xf <= a
        bit = ~off
        y = torch.where(off, b, xf)
    else:
        raise KeyError(name)
    return y.to(x.dtype), bit


def multipliers(name: str, p0: float = 0.0):
    if name == 'hardsigmoid':
        return 0.0, float(_f32(1.0) / _f32(6.0))
    if name == 'leaky_relu':
        return 1.0, float(_f32(p0))
    return 0.0, 1.0


def backward(name: str, gy: torch.Tensor, bit: torch.Tensor, p0: float = 0.0) -> torch.Tensor:
    m0, m1 = multipliers(name, p0)
    m = torch.where(bit, _f32(m1), _f32(m0))
    return (m * gy.detach().cpu().float()).to(gy.dtype)


def pack_bits(bit: torch.Tensor) -> torch.Tensor:
    n = bit.numel()
    padded = torch.zeros((n + 7) // 8 * 8, dtype=torch.int32)
    padded[:n] = bit.to(torch.int32)
    weights = 1 << torch.arange(8, dtype=torch.int32)
    return (padded.view(-1, 8) * weights).sum(1).to(torch.uint8)


def aten(name: str, x: torch.Tensor, p0: float = 0.0, p1: float = 0.0):
    """(y, dy/dx with gy = 1) of ATen's own forward and autograd on the host, in the dtype of x"""
    call = {'hardshrink': lambda t: F.hardshrink(t, p0), 'hardsigmoid': F.hardsigmoid, 'hardtanh': lambda t: F.hardtanh(t, p0, p1),
            'leaky_relu': lambda t: F.leaky_relu(t, p0), 'relu': F.relu, 'relu6': F.relu6, 'softshrink': lambda t: F.softshrink(t, p0),
            'threshold': lambda t: F.threshold(t, p0, p1)}[name]
    t = x.detach().cpu().clone().requires_grad_()
    y = call(t)
    y.backward(torch.ones_like(y))
    return y.detach(), t.grad
