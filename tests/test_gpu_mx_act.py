"""``cabi_x.mx_act_forward`` / ``mx_act_backward`` on the GPU (include/fewbit_hipx.h, "The pre-activation as row blocks"; fewbit_amd/csrc/fewbit_mxact.hip)
against what they are defined by.  Every cell buffer is ``mx_pack`` of its tensor with its seed bit for bit.  16-bit ``h`` and every ``du`` lie within
one unit in the last place of the dtype of the float64 value (an fp32 evaluation to a few fp32 ulps plus one rounding); silu and gelu are the bytes of
``glu_forward(u, ones)``.  fp32 ``h``: the bound ``tests/test_gpu_glu.py`` (``check_y``) holds the fp32 product to -- the largest error in ulps is at most
that of torch's own fp32 activation on the same tensor plus 2.  ``h^`` is never written: it is ``mx_act_forward`` of the decode ``u^``, which every dtype
here holds exactly (checked with ``mx_unpack_host`` for N(0, 1) inputs).
Shapes, the edges of the walk: (70, 200) three row blocks, the last of 6 rows, one full strip of 128 columns and a part of one; (33, 77) an odd width,
element accesses and a pair that straddles the width; (96, 128) a view with row stride 136 that starts one element into its buffer, a misaligned base."""
import pytest
import torch
import torch.nn.functional as F

from fewbit_amd import cabi_x
from test_gpu_mx import DEV, defined, ids

pytestmark = pytest.mark.gpu
SHAPES = ((70, 200, False), (33, 77, False), (96, 128, True))
SEEDS = (0x1234567, 0xfeed5, 0xbeef77)                                       # u, du, h^
MANTISSA = {torch.float32: 23, torch.float16: 10, torch.bfloat16: 7}
TINY = {torch.float32: 2.0**-149, torch.float16: 2.0**-24, torch.bfloat16: 2.0**-133}
every = pytest.mark.parametrize('activation, format, dtype', [(a, f, d) for a in cabi_x.MX_ACTIVATIONS for f in ('fp4', 'fp6') for d in (torch.bfloat16, torch.float16)]
                                + [(a, ('fp4', 'fp6')[i % 2], torch.float32) for i, a in enumerate(cabi_x.MX_ACTIVATIONS)], ids=ids)


def act64(u, activation):
    u = u.double()
    return F.relu(u) if activation == 'relu' else F.silu(u) if activation == 'silu' else F.gelu(u, approximate='tanh' if activation == 'gelu_tanh' else 'none')


def ulp(exact, dtype):
    """one unit in the last place of ``dtype`` at each float64 value (the smallest subnormal at and around 0)"""
    unit = torch.ldexp(torch.ones_like(exact), torch.frexp(exact)[1] - 1 - MANTISSA[dtype])
    return torch.where(exact == 0, torch.zeros_like(exact), unit).clamp_min(TINY[dtype])


def placed(values, strided):
    """``values`` on the device: dense, or (96 x 128) a view with row stride 136 that starts one element into its buffer"""
    if not strided:
        return values.to(DEV)
    view = torch.zeros(values.shape[0] * 136 + 1, dtype=values.dtype, device=DEV)[1:].as_strided(tuple(values.shape), (136, 1))
    return view.copy_(values)


def problem(rows, width, dtype, strided):
    gen = torch.Generator().manual_seed(1000 * rows + width)
    u, gh = (torch.randn(rows, width, generator=gen).to(dtype) for _ in range(2))
    return u, gh, placed(u, strided), placed(gh, strided)


@every
def test_forward_is_the_activation_and_one_mx_pack(activation, format, dtype):
    for rows, width, strided in SHAPES:
        host, _, u, _ = problem(rows, width, dtype, strided)
        h, state = cabi_x.mx_act_forward(u, activation, format, SEEDS[0])
        assert torch.equal(defined(state, rows, width), defined(cabi_x.mx_pack(u, SEEDS[0], format, 'kept'), rows, width)), (rows, width)
        words = torch.tensor(SEEDS[:1], dtype=torch.int64, device=DEV)          # the seed as a word on the device; no buffer: the same h
        assert torch.equal(defined(cabi_x.mx_act_forward(u, activation, format, words)[1], rows, width), defined(state, rows, width))
        plain = cabi_x.mx_act_forward(u, activation, format, keep=False)
        assert plain[1] is None and torch.equal(plain[0].view(torch.uint8), h.view(torch.uint8))
        exact = act64(host, activation)
        error = (h.cpu().double() - exact).abs() / ulp(exact, dtype)
        if dtype == torch.float32:
            own =F.relu if activation == 'relu' else F.silu if activation == 'silu' else (lambda t: F.gelu(t, approximate='tanh' if activation == 'gelu_tanh' else 'none'))
            torchs = (own(host.to(DEV)).cpu().double() - exact).abs() / ulp(exact, dtype)
            print(f'{activation} {rows}x{width} fp32 h: max error {float(error.max()):.2f} ulp, torch {float(torchs.max()):.2f} ulp')
            assert float(error.max()) <= float(torchs.max()) + 2.0, (rows, width)
        else:
            print(f'{activation} {rows}x{width} {dtype} h: max error {float(error.max()):.3f} ulp')
            assert float(error.max()) <= 1.0, (rows, width)
        if activation in ('silu', 'gelu'):
            product = cabi_x.glu_forward(u, torch.ones_like(u), activation, keep=False)[0]
            assert torch.equal(h.contiguous().view(torch.uint8), product.contiguous().view(torch.uint8)), (rows, width)


@every
def test_backward_is_the_slope_on_the_decode_and_two_mx_packs(activation, format, dtype):
    for rows, width, strided in SHAPES:
        _, gh_host, u, gh = problem(rows, width, dtype, strided)
        state = cabi_x.mx_act_forward(u, activation, format, SEEDS[0])[1]
        u_hat = cabi_x.mx_unpack(state, rows, width, format, dtype)
        assert torch.equal(u_hat.cpu().float(), cabi_x.mx_unpack_host(state.cpu(), rows, width, format))       # (the decode is exact in dtype)
        du, du_cells, product_cells = cabi_x.mx_act_backward(gh, state, activation, format, SEEDS[1:])
        u64 = u_hat.cpu().double().requires_grad_()
        want = gh_host.double() * torch.autograd.grad(act64(u64, activation).sum(), u64)[0]
        error = (du.cpu().double() - want).abs() / ulp(want, dtype)
        print(f'{activation} {format} {rows}x{width} {dtype} du: max error {float(error.max()):.3f} ulp')
        assert float(error.max()) <= 1.0, (rows, width)
        assert torch.equal(defined(du_cells, rows, width), defined(cabi_x.mx_pack(du, SEEDS[1], 'fp8', 'grad'), rows, width)), (rows, width)
        h_hat = cabi_x.mx_act_forward(u_hat, activation, format, keep=False)[0]
        assert torch.equal(defined(product_cells, rows, width), defined(cabi_x.mx_pack(h_hat, SEEDS[2], format, 'kept'), rows, width)), (rows, width)
        # the seeds as words on the device; each output absent in turn: None, and a buffer filled with a sentinel is untouched
        words = torch.tensor(SEEDS[1:], dtype=torch.int64, device=DEV)
        for absent in range(3):
            buffers = (torch.full_like(du, 7.0), torch.full_like(du_cells, 0xA5), torch.full_like(product_cells, 0xA5))
            outs = cabi_x.mx_act_backward(gh, state, activation, format, words, [i != absent for i in range(3)], *buffers)
            for i, (out, buffer, first) in enumerate(zip(outs, buffers, (du, du_cells, product_cells))):
                if i == absent:
                    assert out is None and bool((buffer == (7.0 if i == 0 else 0xA5)).all())
                elif i == 0:
                    assert torch.equal(out.view(torch.uint8), first.contiguous().view(torch.uint8))
                else:
                    assert torch.equal(defined(out, rows, width), defined(first, rows, width))


def test_a_poisoned_state_cell_is_nan_on_its_rows_of_its_column_and_nowhere_else():
    rows, width = 70, 200
    host, _, _, gh = problem(rows, width, torch.bfloat16, False)
    host[40, 5] = float('inf')
    state = cabi_x.mx_act_forward(host.to(DEV), 'gelu', 'fp6', SEEDS[0])[1]
    assert int(state[1 * width + 5]) == 0xFF
    du, _, product_cells = cabi_x.mx_act_backward(gh, state, 'gelu', 'fp6', SEEDS[1:])
    nan = torch.zeros(rows, width, dtype=torch.bool, device=DEV)
    nan[32:64, 5] = True
    for got in (du, cabi_x.mx_unpack(product_cells, rows, width, 'fp6', torch.bfloat16)):
        assert torch.equal(got.isnan(), nan) and bool(torch.isfinite(got[~nan]).all())
