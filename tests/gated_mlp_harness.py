"""What the tests of the gated MLP as one node share (tests/test_gated_mlp_host.py, test_gpu_glu_product.py, test_gpu_gated_mlp_layer.py): the two
neighbouring levels of every element and inputs whose rounding has a variance worth the name (both restated from tests/test_glu_host.py), a
Llama-style stub, and the composition of the entry points the node stands for."""
import numpy as np
import torch
import torch.nn.functional as F


# ---- the expectation of a rounded element -------------------------------------------------------------------------------------------------------
def levels_of(x, lo, step, bits):
    """(v0, v1, f) of every element, float64: the two neighbouring decodes and the probability of the upper one, from lo, step and the fp32 t of the
    definition (include/fewbit_hipx.h, "the packed form of a seed")"""
    L = np.float32(2**bits - 1)
    lo, step = np.repeat(lo, 64)[:x.size], np.repeat(step, 64)[:x.size]
    with np.errstate(all='ignore'):
        hi = np.array([x[i:i + 64].max() for i in range(0, x.size, 64)], dtype=np.float32)
        rng = (np.repeat(hi, 64)[:x.size] - lo).astype(np.float32)
        inv = np.where(rng > 0, (L / rng).astype(np.float32), np.float32(0))
    t = ((x - lo).astype(np.float32) * inv).astype(np.float32)
    k = np.minimum(np.floor(t), L - 1).astype(np.float64)          # (the maximum of a group: t = L exactly, code L with certainty -- f = 1 over level L - 1)
    f = t.astype(np.float64) - k
    fma = lambda code: (code * step.astype(np.float64) + lo.astype(np.float64)).astype(np.float32).astype(np.float64)
    return fma(k), fma(k + 1), f


def tame(x, bits, generator):
    """`x` with every element but its group's minimum and maximum moved to a level plus a fraction in [0.15, 0.85] of a step: every variance that is
    not exactly 0 is then at least 0.1275 step^2, far above the 2^-16 granularity of U"""
    x = x.clone().view(-1, 64)
    L = 2**bits - 1
    lo, hi = x.amin(dim=1, keepdim=True), x.amax(dim=1, keepdim=True)
    step = (hi - lo) / L
    k = torch.randint(0, L, x.shape, generator=generator)
    f = 0.15 + 0.7 * torch.rand(x.shape, generator=generator)
    moved = lo + (k + f) * step
    keep = (x == lo) | (x == hi)
    return torch.where(keep, x, moved).reshape(-1)


# ---- guarded, strided buffers on the GPU (restated from tests/test_gpu_glu.py) ------------------------------------------------------------------------
class Strided:
    """a logical rows x width matrix whose rows are `ld` elements apart, `off` elements behind a 256-byte aligned address, in a guarded buffer that
    ends with the last element of the last row; every byte of it is the sentinel until `values` are written"""

    def __init__(self, rows, width, ld, dtype, off=0, values=None):
        from norm_harness import Guarded
        self.buffer = Guarded((rows - 1) * ld + width, dtype, off)
        self.view = self.buffer.t.as_strided((rows, width), (ld, 1))
        if values is not None:
            self.view.copy_(values)
            self.buffer.before = self.buffer.raw.clone()

    def only_the_matrix_was_written(self):
        """the guards, and the gaps between the rows, hold what they held"""
        after = self.buffer.raw.clone()
        was = self.buffer.before[self.buffer.lo:self.buffer.hi].view(self.view.dtype).as_strided(self.view.shape, self.view.stride())
        after[self.buffer.lo:self.buffer.hi].view(self.view.dtype).as_strided(self.view.shape, self.view.stride()).copy_(was)
        return torch.equal(after, self.buffer.before)

    def unchanged(self):
        return self.buffer.unchanged()


def inputs(rows, width, dtype, salt=0):
    """(gate, up, gy) on the host, 3 N(0, 1) each, rounded to `dtype`: as tests/test_gpu_glu.py draws them"""
    g = torch.Generator().manual_seed(1000 * rows + width + salt)
    return tuple((3 * torch.randn(rows, width, generator=g)).to(dtype) for _ in range(3))


def within_16_bit_bound(got, exact, dtype):
    """|got - exact| <= (half an ulp + the fp32 error allowed to act) |exact| + the smallest subnormal: the bound tests/test_gpu_glu.py holds y to"""
    from glu_harness import FAST_CLASS, TINY, UNIT
    return (got.double() - exact).abs() <= UNIT[dtype] * exact.abs() + FAST_CLASS * exact.abs() + TINY[dtype]


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


# ---- a gated MLP as models spell it ---------------------------------------------------------------------------------------------------------------
class StubMLP(torch.nn.Module):
    """the MLP of a Llama-style model"""

    def __init__(self, act_fn, width=16, hidden=40, bias=False, device=None, dtype=None):
        super().__init__()
        self.gate_proj = torch.nn.Linear(width, hidden, bias=bias, device=device, dtype=dtype)
        self.up_proj = torch.nn.Linear(width, hidden, bias=bias, device=device, dtype=dtype)
        self.down_proj = torch.nn.Linear(hidden, width, bias=bias, device=device, dtype=dtype)
        self.act_fn = act_fn

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


class StubBlock(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.norm = torch.nn.LayerNorm(16)
        self.mlp = StubMLP(torch.nn.SiLU())

    def forward(self, x):
        return x + self.mlp(self.norm(x))


def exact_mlp(x, mlp, activation):
    """``down(act(gate(x)) * up(x))`` with ``F.linear`` and torch's own product"""
    gate, up = F.linear(x, mlp.gate_proj.weight, mlp.gate_proj.bias), F.linear(x, mlp.up_proj.weight, mlp.up_proj.bias)
    return F.linear((F.silu(gate) if activation == 'silu' else F.gelu(gate)) * up, mlp.down_proj.weight, mlp.down_proj.bias)


def parameters_of(mlp):
    """(name, parameter) of the projections, biases included where they exist, in the order gate, up, down"""
    return [(f'{name}.{kind}', getattr(getattr(mlp, name), kind)) for name in ('gate_proj', 'up_proj', 'down_proj') for kind in ('weight', 'bias')
            if getattr(getattr(mlp, name), kind) is not None]
