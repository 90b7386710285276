"""What the cross-entropy tests share (tests/test_gpu_cross_entropy.py, tests/test_gpu_cross_entropy_layer.py): the bounds of include/fewbit_hipx.h
("The loss of a row"), logits placed in a guarded buffer at a chosen offset and row stride, and the comparison with the float64 host evaluation.

The bounds are derived, not tuned, for |x| <= 16 (so |x - max| <= 32).  S = sum exp(x_j - M) in [1, V] is a sum of positive terms: in any order its
relative error is at most (V - 1) 2^-24 plus that of a term, and a term's is at most (2.5 |x - M| + 4) 2^-24 <= 128 2^-24 (the rounding of the
difference, of the product with log2 e, and v_exp_f32 itself).  Hence against float64, with E = (V + 128) 2^-24 + 4 2^-24 |lse64|:
    |lse - lse64| <= E,    |loss - loss64| <= E + 4 2^-24 (|lse64| + |x_t|),
    |d - d64| <= |g| (p64 (E + 160 2^-24) + 2^-23) + r |d64|,   r = 0 (fp32), 2^-11 (+ 2^-25 absolute, fp16), 2^-8 (bf16)."""
import torch

from fewbit_amd import cabi_x

U = 2.0**-24
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
ROUNDING = {torch.float32: (0.0, 0.0), torch.float16: (2.0**-11, 2.0**-25), torch.bfloat16: (2.0**-8, 0.0)}
GUARD = 64                                                  # elements in front of and behind the rows


def bound_lse(width, lse64):
    return (width + 128) * U + 4 * U * lse64.abs()


def draw(rows, width, dtype, salt=0):
    """values in [-16, 16] that the dtype holds exactly, targets, one gradient per row (of both signs)"""
    g = torch.Generator().manual_seed(1000 * salt + width)
    x = (torch.rand(rows, width, generator=g) * 32 - 16).to(dtype)
    t = torch.randint(0, width, (rows, ), generator=g)
    grow = (torch.randn(rows, generator=g) * 2).to(torch.float32)
    return x, t, grow


class Placed:
    """``values`` (a host ``rows x width`` tensor) on the device inside a buffer of a recognisable filling: ``view`` is the logits, ``offset`` elements
    behind a 16-byte boundary, rows ``ld`` elements apart.  ``untouched()`` says whether everything around the rows still has its filling."""

    def __init__(self, values, ld=None, offset=1, device='cuda'):
        rows, width = values.shape
        ld = width if ld is None else ld
        self.start, self.rows, self.width, self.ld = GUARD + offset, rows, width, ld
        filling = torch.full((self.start + rows * ld + GUARD, ), 13.0, dtype=values.dtype)
        self.raw = filling.to(device)
        assert self.raw.data_ptr() % 16 == 0
        self.view = self.raw.as_strided((rows, width), (ld, 1), self.start)
        self.view.copy_(values.to(device))
        outside = torch.ones(self.raw.numel(), dtype=torch.bool)
        for r in range(rows):
            outside[self.start + r * ld:self.start + r * ld + width] = False
        self.outside = outside.to(device)

    def untouched(self):
        return bool((self.raw[self.outside] == 13.0).all())

    def empty_like(self, offset=None, ld=None):
        """a guarded buffer for an output of the same shape (by default at the same offset and row stride: the 16-byte stores)"""
        blank = torch.zeros(self.rows, self.width, dtype=self.raw.dtype)
        return Placed(blank, self.ld if ld is None else ld, self.start - GUARD if offset is None else offset, self.raw.device)


def bits(t):
    """the elements as integers: equal means the same bits, NaN included"""
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def reference(view, t, grow, ignore_index=-100):
    """the float64 host evaluation of the device logits ``view``"""
    g = None if grow is None else grow.detach().cpu().double().reshape(-1)
    return cabi_x.cross_entropy_host(view.detach().float().cpu(), t.cpu(), ignore_index, g)


def within(got, want, bound, what):
    """``got`` (fp32 or the dtype, on the device) against the float64 ``want``: NaN exactly where it is NaN, infinities equal, the rest within ``bound``"""
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (what, 'NaN in other places')
    infinite = torch.isinf(want)
    assert torch.equal(got[infinite], want[infinite]), (what, 'infinities')
    finite = torch.isfinite(want)
    err, room = (got[finite] - want[finite]).abs(), bound.expand_as(want)[finite]
    worst = float((err / room.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert worst <= 1.0, (what, f'{worst:.3f} of the bound', float(err.max()))
    return worst


def check(view, t, grow, lse, loss, d, ignore_index=-100):
    """every lse, loss and gradient of one call against the bounds of the header; returns the worst fractions of the three bounds"""
    width = view.shape[1]
    lse64, loss64, d64 = reference(view, t, grow, ignore_index)
    x64 = view.detach().double().cpu()
    g = torch.ones(view.shape[0], dtype=torch.float64) if grow is None else grow.detach().double().cpu().reshape(-1).expand(view.shape[0])
    safe = torch.where(torch.isfinite(lse64), lse64, torch.zeros_like(lse64))
    e = bound_lse(width, safe)
    a = within(lse, lse64, e, 'lse')
    valid = (t.cpu() >= 0) & (t.cpu() < width)
    xt = x64.gather(1, t.cpu().clamp(0, width - 1)[:, None])[:, 0]
    xt = torch.where(valid & torch.isfinite(xt), xt, torch.zeros_like(xt))
    b = within(loss, loss64, e + 4 * U * (safe.abs() + xt.abs()), 'loss')
    assert not torch.signbit(loss.detach().cpu()[t.cpu() == ignore_index]).any()
    p64 = torch.exp(x64 - safe[:, None])
    p64 = torch.where(torch.isfinite(p64), p64, torch.zeros_like(p64))
    rel, absolute = ROUNDING[view.dtype]
    room = g.abs()[:, None] * (p64 * (e[:, None] + 160 * U) + 2 * U) + rel * d64.abs().nan_to_num(0.0, 0.0, 0.0) + absolute
    c = within(d, d64, room, 'dlogits')
    # exactly +0: ignored rows, and -inf elements that are not the target of their row
    dc, tc = d.detach().cpu(), t.cpu()
    zero = (x64 == float('-inf')) & ~torch.isnan(d64)
    zero[torch.arange(len(tc))[valid], tc[valid]] = False
    zero[tc == ignore_index] = True
    assert not dc[zero].any() and not torch.signbit(dc[zero]).any(), 'a gradient that must be +0 is not'
    return a, b, c
