"""The sum of a seed in front of the centred normalized rows without a GPU (fewbit_amd/csrc/fewbit_mxlnorm.hip): the two symbols, the refusals, and the
host evaluation against float64 on the decoded cells."""
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from fewbit_amd import cabi_x

NAMES = ('fewbit_hipx_mx_add_layer_norm_forward', 'fewbit_hipx_mx_add_layer_norm_backward')
P = 4096                                                                  # a pointer that is never followed: every call below is refused before a launch
Q = P + 40 * 24 * 2                                                       # a second matrix behind the first
CELLS, WORKSPACE = cabi_x.mx_bytes(40, 24, 'fp4'), 2 * 2 * 24 * 4
FORWARD = dict(dtype=2, x=P, ld_x=24, residual=P, ld_residual=24, rows=40, width=24, gamma=P, beta=P, eps=1e-5, format=4, seed=1, seed_mask=2, word=None,
               threshold=6554, y=P, ld_y=24, h=Q, ld_h=24, mean=P, rstd=P, cells=P, cells_bytes=CELLS, stream=None)
BACKWARD = dict(dtype=2, gy=P, ld_gy=24, gy_add=P, ld_gy_add=24, gh=P, ld_gh=24, cells=P, cells_bytes=CELLS, rstd=P, gamma=P, rows=40, width=24, format=4,
                seed_mask=2, word=None, threshold=6554, dres=P, ld_dres=24, dbranch=Q, ld_dbranch=24, dgamma=P, dbeta=P, workspace=P,
                workspace_bytes=WORKSPACE, stream=None)
REFUSALS = [('mx_add_layer_norm_forward', FORWARD, change, text) for change, text in (
    (dict(dtype=99), 'unknown dtype'), (dict(format=8), 'format'), (dict(word=P + 4), 'seed word'), (dict(rows=0), 'rows'),
    (dict(width=8193, ld_x=8193, ld_residual=8193, ld_y=8193, ld_h=8193), 'width'), (dict(threshold=65537), 'threshold'),
    (dict(width=13), 'multiple of 8'), (dict(residual=None), 'null pointer (residual)'), (dict(x=None), 'null'), (dict(ld_residual=23), 'ld'),
    (dict(ld_h=23), 'ld'), (dict(residual=P + 1), 'element'), (dict(h=P + 1), 'element'), (dict(mean=P + 2), 'element'), (dict(cells=P + 8), '16-byte'),
    (dict(cells_bytes=CELLS - 1), 'bytes'), (dict(h=Q - 2), 'overlap'), (dict(h=P + 48, ld_y=48, ld_h=47), 'overlap'))]
REFUSALS += [('mx_add_layer_norm_backward', BACKWARD, change, text) for change, text in (
    (dict(dtype=99), 'unknown dtype'), (dict(format=5), 'format'), (dict(word=P + 4), 'seed word'), (dict(threshold=65537), 'threshold'),
    (dict(width=13), 'multiple of 8'), (dict(threshold=0), 'dbranch is dres'), (dict(gy=None), 'null'), (dict(workspace=None), 'null'), (dict(ld_gy_add=23), 'ld'),
    (dict(ld_dbranch=23), 'ld'), (dict(gy_add=P + 1), 'element'), (dict(dbeta=P + 2), 'element'), (dict(cells_bytes=CELLS - 1), 'bytes'),
    (dict(workspace_bytes=WORKSPACE - 1), 'bytes'), (dict(dbranch=P), 'overlap'))]


@pytest.mark.parametrize('name, base, change, text', REFUSALS)
def test_what_the_entry_points_refuse_before_anything_is_launched(name, base, change, text):
    rc = getattr(cabi_x.lib(), 'fewbit_hipx_' + name)(*{**base, **change}.values())
    message = cabi_x.lib().fewbit_hipx_last_error().decode()
    assert rc != 0 and message.startswith(name) and text in message


def test_the_names():
    header, exported = (Path(__file__).resolve().parent.parent / 'include' / 'fewbit_hipx.h').read_text(), cabi_x.lib()
    assert all(name + '(' in header and name in cabi_x.SYMBOLS and hasattr(exported, name) for name in NAMES) and exported.fewbit_hipx_revision() == 2
    assert all(name[len('fewbit_hipx_'):] in cabi_x.__all__ for name in NAMES) and cabi_x.MX_NORM_PLAN_WIDTHS == ()


@pytest.mark.parametrize('rows, width, p', ((33, 72, 0.1), (65, 13, 0.0)))
@pytest.mark.parametrize('format', ('fp4', 'fp6'))
def test_the_host_evaluation_against_float64_on_the_decoded_cells(format, rows, width, p):
    """fp32 torch against the same expressions in float64, u = 2^-24, n = width.  h: three roundings (scale, product, sum), 4 u of the larger operand.
    y from the rounded h: the mean (n + 1 operations) and the centred squares (n + 2 more) under a square root, then four operations: (n + 8) u of
    (|h - mean| + |mean|) rstd |gamma| + u |beta|.  dx = rstd ((g^ - c1) - x^q c2) on the decoded x^q: (n + 8) u of rstd (|g^| + mean|g^| + |x^q|
    mean|g^ x^q|); gy_add and gh add 2 u each of their sums, the scale 4 u.  dgamma, dbeta: `rows` terms, (rows + 1) u of the sum of magnitudes."""
    gen, u, n = torch.Generator().manual_seed(7 + width), 2.0**-24, width
    x, r, gy, gh, at_y = (torch.randn(rows, width, generator=gen) for _ in range(5))
    gamma, beta = 1 + 0.5 * torch.randn(width, generator=gen), torch.randn(width, generator=gen)
    y, cells, rstd, h, mean = cabi_x.mx_add_layer_norm_host(x, r, gamma, beta, 1e-5, format, (11, 12), p)
    t = cabi_x.dropout_threshold(p)
    keep, scale = cabi_x.dropout_keep(12, rows * width, p).view(rows, width), 65536.0 / (65536 - t)
    h64 = r.double() + keep * x.double() * scale
    assert (0 < int((~keep).sum()) < rows * width // 4) == (t > 0) and float((h.double() - h64).abs().max()) <= 4 * u * max(float(x.abs().max()) * scale, float(h64.abs().max()))
    hd, m64 = h.double(), h.double().mean(dim=1, keepdim=True)
    r64 = 1.0 / torch.sqrt((hd - m64).square().mean(dim=1, keepdim=True) + 1e-5)
    bound = (n + 8) * u * ((hd - m64).abs() + m64.abs()) * r64 * gamma.double().abs() + u * beta.double().abs()
    assert bool(((y.double() - F.layer_norm(hd, (width, ), gamma.double(), beta.double(), 1e-5)).abs() <= bound).all())
    assert bool(((rstd.double()[:, None] - r64).abs() <= (n + 8) * u * r64).all()) and bool(((mean.double()[:, None] - m64).abs() <= (n + 1) * u * hd.abs().mean(dim=1, keepdim=True)).all())
    xq, rs = cabi_x.mx_unpack_host(cells, rows, width, format).double(), rstd.double()[:, None]
    g64 = gy.double() + at_y.double()
    g = g64 * gamma.double()
    c1, c2 = g.mean(dim=1, keepdim=True), (g * xq).mean(dim=1, keepdim=True)
    dres64 = rs * ((g - c1) - xq * c2) + gh.double()
    bound = (n + 8) * u * rs * (g.abs() + g.abs().mean(dim=1, keepdim=True) + xq.abs() * (g * xq).abs().mean(dim=1, keepdim=True)) + 4 * u * (dres64.abs() + gh.double().abs())
    dres, dbranch, dgamma, dbeta = cabi_x.mx_add_layer_norm_backward_host(gy, cells, rstd, gamma, format, 12, p, gh, at_y)
    assert bool(((dres.double() - dres64).abs() <= bound).all())
    assert bool(((dbranch.double() - keep * dres64 * scale).abs() <= scale * (bound + 4 * u * dres64.abs())).all()) and bool((dbranch[~keep] == 0).all())
    assert bool(((dgamma.double() - (g64 * xq).sum(dim=0)).abs() <= (rows + 3) * u * (g64 * xq).abs().sum(dim=0)).all())
    assert bool(((dbeta.double() - g64.sum(dim=0)).abs() <= (rows + 3) * u * g64.abs().sum(dim=0)).all())
