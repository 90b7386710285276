"""The gate and the up as row blocks without a GPU (include/fewbit_hipx.h; fewbit_amd/csrc/fewbit_mxglu.hip): what the two entry points refuse before
anything is launched, and ``fewbit.functional.gated_mlp_mx`` on host tensors -- the composed route -- against a float64 MLP at the layer shape of
tests/test_gpu_mx_gated_mlp.py.

The bound of the host route.  Every kept element is rounded to a neighbour of its format's grid without bias, so its error is below one spacing and its
RMS error below half of one; relative to the largest elements of a cell the spacing is 2^-M (M mantissa bits: 1 at fp4, 3 at fp6) and smaller
elements sit on finer grids.  A gradient here is a product of up to three such tensors (x^, g^, u^) summed over 96 rows with independent errors, whose
relative errors add in squares: sqrt(3) * 2^-M / 2 < 2^-M bounds the relative Frobenius error of each gradient."""
import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi_x

P = 4096                                                                  # a pointer that is never followed: every call below is refused before a launch
STATE = cabi_x.mx_glu_state_bytes(40, 24, 'fp4')
FORWARD = dict(dtype=2, act=2, gate=P, ld_gate=24, up=P, ld_up=24, rows=40, width=24, format=4, seed_gate=1, seed_up=2, word=None, y=P, ld_y=24, state=P,
               state_bytes=STATE, stream=None)
BACKWARD = dict(dtype=2, act=2, gy=P, ld_gy=24, state=P, state_bytes=STATE, rows=40, width=24, format=4, seed_dgate=1, seed_dup=2, seed_product=3, word=None,
                d_gate=P, ld_dgate=24, d_up=P, ld_dup=24, d_gate_cells=P, d_up_cells=P, product_cells=P, stream=None)
REFUSALS = [('mx_glu_forward', FORWARD, change, text) for change, text in (
    (dict(dtype=99), 'unknown dtype'), (dict(act=0), 'activation'), (dict(format=8), 'format'), (dict(word=P + 4), 'seed word'), (dict(width=2**23 + 1), '2^23'),
    (dict(gate=None), 'null'), (dict(y=None), 'null'), (dict(state=None), 'null'), (dict(ld_up=23), 'ld'), (dict(ld_y=23), 'ld'), (dict(up=P + 1), 'element'),
    (dict(state=P + 8), '16-byte'), (dict(state_bytes=STATE - 1), 'bytes'))]
REFUSALS += [('mx_glu_backward', BACKWARD, change, text) for change, text in (
    (dict(dtype=99), 'unknown dtype'), (dict(act=0), 'activation'), (dict(format=8), 'format'), (dict(word=P + 4), 'seed word'),
    (dict(rows=2**30, width=2**20), '2^36'), (dict(gy=None), 'null'), (dict(state=None), 'null'), (dict(ld_gy=23), 'ld'), (dict(ld_dup=23), 'ld'),
    (dict(d_gate=P + 1), 'element'), (dict(state=P + 8), '16-byte'), (dict(d_up_cells=P + 8), '16-byte'), (dict(product_cells=P + 8), '16-byte'),
    (dict(state_bytes=STATE - 1), 'bytes'))]


@pytest.mark.parametrize('name, base, change, text', REFUSALS)
def test_what_the_entry_points_refuse_before_anything_is_launched(name, base, change, text):
    rc = getattr(cabi_x.lib(), 'fewbit_hipx_' + name)(*{**base, **change}.values())
    assert rc != 0 and text in cabi_x.lib().fewbit_hipx_last_error().decode()
    assert getattr(cabi_x.lib(), 'fewbit_hipx_' + name)(*{**base, 'rows': 0}.values()) == 0            # no elements: nothing to do


def test_the_state_is_two_aligned_buffers_and_the_names_are_exported():
    for rows, width, format in ((1, 8, 'fp4'), (33, 72, 'fp6'), (65, 200, 'fp6'), (33, 1, 'fp6')):
        assert cabi_x.mx_glu_state_bytes(rows, width, format) == 2 * (-(-cabi_x.mx_bytes(rows, width, format) // 16) * 16)
    assert cabi_x.mx_glu_state_bytes(4, 4, 'fp8') == 0 and cabi_x.mx_glu_state_bytes(1, 2**23 + 1, 'fp4') == 0
    assert fewbit.MXGatedMLP is fewbit.glu.MXGatedMLP and fewbit.functional.gated_mlp_mx is fewbit.glu.gated_mlp_mx


@pytest.mark.parametrize('activation', ('silu', 'gelu'))
@pytest.mark.parametrize('format, bound', (('fp4', 0.5), ('fp6', 0.125)))
def test_the_host_route_against_float64_at_the_layer_shape(format, bound, activation):
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(96, 64, generator=gen, requires_grad=True)
    weights = [(torch.randn(s, generator=gen) * s[1]**-0.5).requires_grad_() for s in ((96, 64), (96, 64), (64, 96))]
    gy = torch.randn(96, 64, generator=gen)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        out = fewbit.functional.gated_mlp_mx(x, *weights, activation=activation, format=format, generator=torch.Generator().manual_seed(11))
    got = torch.autograd.grad(out, (x, *weights), gy)
    x64, (wg, wu, wd) = x.detach().double().requires_grad_(), [w.detach().double().requires_grad_() for w in weights]
    act = F.silu if activation == 'silu' else F.gelu
    want = torch.autograd.grad(F.linear(act(F.linear(x64, wg)) * F.linear(x64, wu), wd), (x64, wg, wu, wd), gy.double())
    errors = [float((a.double() - b).norm() / b.norm()) for a, b in zip(got, want)]
    print(f'{format} {activation}: relative errors of dx, dWg, dWu, dWd {errors}')
    assert max(errors) <= bound and float((out.detach().double() - F.linear(act(F.linear(x64, wg)) * F.linear(x64, wu), wd).detach()).norm()) <= 1e-5 * float(out.detach().norm())
    # kept: three uint8 buffers (x^, g^, u^) and the weights; nothing of the shape of x, gate or up in a float dtype
    assert sorted(t.numel() for t in saved if t.dtype == torch.uint8) == sorted(cabi_x.mx_bytes(96, w, format) for w in (64, 96, 96))
    assert not any(t.dtype != torch.uint8 and t.shape[0] == 96 and t.shape != (96, 64) for t in saved) and sum(t.shape == (96, 64) for t in saved) == 2
    with pytest.raises(ValueError):
        fewbit.functional.gated_mlp_mx(x, *weights, format='fp8')
