"""The sum of a seed in front of the normalized rows without a GPU (fewbit_amd/csrc/fewbit_mxnorm.hip): the two symbols, the refusals, the host evaluation
against float64 on the decoded cells, ``fewbit.functional.rms_norm_linear_mx`` with a residual on host tensors, and the unchanged default call."""
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi_x

NAMES = ('fewbit_hipx_mx_add_rms_norm_forward', 'fewbit_hipx_mx_add_rms_norm_backward')
P = 4096                                                                  # a pointer that is never followed: every call below is refused before a launch
CELLS, WORKSPACE = cabi_x.mx_bytes(40, 24, 'fp4'), 2 * 24 * 4
FORWARD = dict(dtype=2, x=P, ld_x=24, residual=P, ld_residual=24, rows=40, width=24, gamma=P, eps=1e-5, format=4, seed=1, seed_mask=2, word=None, threshold=6554,
               y=P, ld_y=24, h=P, ld_h=24, rstd=P, cells=P, cells_bytes=CELLS, stream=None)
BACKWARD = dict(dtype=2, gy=P, ld_gy=24, gh=P, ld_gh=24, cells=P, cells_bytes=CELLS, rstd=P, gamma=P, rows=40, width=24, format=4, seed_mask=2, word=None,
                threshold=6554, dres=P, ld_dres=24, dbranch=P, ld_dbranch=24, dgamma=P, workspace=P, workspace_bytes=WORKSPACE, stream=None)
REFUSALS = [('mx_add_rms_norm_forward', FORWARD, change, text) for change, text in (
    (dict(dtype=99), 'unknown dtype'), (dict(format=8), 'format'), (dict(word=P + 4), 'seed word'), (dict(rows=0), 'rows'),
    (dict(width=8193, ld_x=8193, ld_residual=8193, ld_y=8193, ld_h=8193), 'width'), (dict(threshold=65537), 'threshold'),
    (dict(width=13), 'multiple of 8'), (dict(residual=None), 'null pointer (residual)'), (dict(x=None), 'null'), (dict(ld_residual=23), 'ld'),
    (dict(ld_h=23), 'ld'), (dict(residual=P + 1), 'element'), (dict(h=P + 1), 'element'), (dict(cells=P + 8), '16-byte'), (dict(cells_bytes=CELLS - 1), 'bytes'))]
REFUSALS += [('mx_add_rms_norm_backward', BACKWARD, change, text) for change, text in (
    (dict(dtype=99), 'unknown dtype'), (dict(format=5), 'format'), (dict(word=P + 4), 'seed word'), (dict(threshold=65537), 'threshold'),
    (dict(width=13), 'multiple of 8'), (dict(threshold=0), 'dbranch is dres'), (dict(gy=None), 'null'), (dict(workspace=None), 'null'), (dict(ld_gh=23), 'ld'),
    (dict(ld_dbranch=23), 'ld'), (dict(gh=P + 1), 'element'), (dict(cells_bytes=CELLS - 1), 'bytes'), (dict(workspace_bytes=WORKSPACE - 1), 'bytes'))]


@pytest.mark.parametrize('name, base, change, text', REFUSALS)
def test_what_the_entry_points_refuse_before_anything_is_launched(name, base, change, text):
    rc = getattr(cabi_x.lib(), 'fewbit_hipx_' + name)(*{**base, **change}.values())
    message = cabi_x.lib().fewbit_hipx_last_error().decode()
    assert rc != 0 and message.startswith(name) and text in message


def test_the_names():
    header, exported = (Path(__file__).resolve().parent.parent / 'include' / 'fewbit_hipx.h').read_text(), cabi_x.lib()
    assert all(name + '(' in header and name in cabi_x.SYMBOLS and hasattr(exported, name) for name in NAMES) and exported.fewbit_hipx_revision() == 2
    assert all(name[len('fewbit_hipx_'):] in cabi_x.__all__ for name in NAMES) and cabi_x.MX_NORM_PLAN_WIDTHS == ()


def leaves(dtype=torch.float32):
    gen = torch.Generator().manual_seed(7)
    shapes = ((65, 64), (65, 64), (64, ), (96, 64), (32, 64), (96, ))
    return [((1.0 if s == (64, ) else 0.0) + 0.5 * torch.randn(s, generator=gen)).to(dtype).requires_grad_() for s in shapes], gen


@pytest.mark.parametrize('format', ('fp4', 'fp6'))
def test_the_host_evaluation_against_float64_on_the_decoded_cells(format):
    """fp32 torch against the same expressions in float64, u = 2^-24.  h: three roundings (scale, product, sum), 4 u of the larger operand.  y from the
    rounded h: every error multiplies, 64 squares added and eight more operations, 72 u.  dx = rstd (g^ - x^q c) on the decoded x^q: 72 u of rstd (|g^| +
    |x^q| mean|g^ x^q|), test_gpu_rms_norm.py's unit with the worst case for its factor; gh adds 2 u of dres, the scale 4 u.  dgamma: 65 rows, 66 u."""
    (x, r, gamma, *_), gen = leaves()
    x, r, gamma = x.detach(), r.detach(), gamma.detach()
    gy, gh, u = torch.randn(65, 64, generator=gen), torch.randn(65, 64, generator=gen), 2.0**-24
    y, cells, rstd, h = cabi_x.mx_add_rms_norm_host(x, r, gamma, 1e-5, format, (11, 12), 0.1)
    keep, scale = cabi_x.dropout_keep(12, 65 * 64, 0.1).view(65, 64), 65536.0 / (65536 - cabi_x.dropout_threshold(0.1))
    h64 = r.double() + keep * x.double() * scale
    assert 0 < int((~keep).sum()) < 65 * 64 // 4 and float((h.double() - h64).abs().max()) <= 4 * u * max(float(x.abs().max()) * scale, float(h64.abs().max()))
    torch.testing.assert_close(y.double(), F.rms_norm(h.double(), (64, ), gamma.double(), 1e-5), rtol=72 * u, atol=0)
    xq, r64 = cabi_x.mx_unpack_host(cells, 65, 64, format).double(), rstd.double()[:, None]
    g = gy.double() * gamma.double()
    dres64 = r64 * (g - xq * (g * xq).mean(dim=1, keepdim=True)) + gh.double()
    bound = 72 * u * r64 * (g.abs() + xq.abs() * (g * xq).abs().mean(dim=1, keepdim=True)) + 2 * u * dres64.abs()
    dres, dbranch, dgamma = cabi_x.mx_add_rms_norm_backward_host(gy, cells, rstd, gamma, format, 12, 0.1, gh)
    assert bool(((dres.double() - dres64).abs() <= bound).all())
    assert bool(((dbranch.double() - keep * dres64 * scale).abs() <= scale * (bound + 4 * u * dres64.abs())).all()) and bool((dbranch[~keep] == 0).all())
    assert bool(((dgamma.double() - (gy.double() * xq).sum(dim=0)).abs() <= 66 * u * (gy.double() * xq).abs().sum(dim=0)).all())


def test_the_node_with_a_residual_on_host_tensors_and_the_default_call():
    """Host tensors ARE the composition: ``dropout_add`` (torch's mask here) and the call without a residual."""
    (x, r, gamma, w0, w1, b0), gen = leaves()
    call = lambda **more: fewbit.functional.rms_norm_linear_mx(x, gamma, (w0, w1), (b0, None), 1e-5, 'fp6', **more)
    torch.manual_seed(5)
    outs = call(residual=r, p=0.25, prenorm=True)
    torch.manual_seed(5)
    h = r + F.dropout(x, 0.25)
    assert len(outs) == 3 and torch.equal(outs[2], h) and outs[0].grad_fn.name() == '_RMSNormLinearMXBackward'
    y = F.rms_norm(h, (64, ), gamma, 1e-5)
    for out, w, b in zip(outs, (w0, w1), (b0, None)):
        torch.testing.assert_close(out, F.linear(y, w, b), rtol=1e-5, atol=1e-5)
    grads = [torch.randn(65, n, generator=gen) for n in (96, 32, 64)]
    dx, dr, db = torch.autograd.grad(outs, (x, r, b0), grads)
    assert torch.equal(db, grads[0].sum(dim=0))
    torch.testing.assert_close(dx, torch.where(h == r, 0.0, dr / 0.75))     # the mask and its scale behind the sum's gradient
    assert len(call(residual=r, training=False)) == 2
    torch.manual_seed(5)
    a = call()
    torch.manual_seed(5)
    b = fewbit.functional.rms_norm_linear_mx(x, gamma, (w0, w1), (b0, None), 1e-5, 'fp6', None, None, 0.0, True, False)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and a[0].grad_fn.name() == '_RMSNormLinearMXBackward'
    with pytest.raises(ValueError):
        call(residual=r[:1])
