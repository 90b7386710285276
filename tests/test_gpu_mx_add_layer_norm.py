"""The fused pair of fewbit_amd/csrc/fewbit_mxlnorm.hip (cabi_x.mx_add_layer_norm_forward / mx_add_layer_norm_backward) against its definition
(include/fewbit_hipx.h, "The sum of a seed in front of the centred normalized rows"): every output bit for bit what the kernels it replaces give --
cabi_x.dropout_apply with the residual as addend, then cabi_x.mx_layer_norm_forward / mx_layer_norm_backward, then torch's adds and the mask.  The
shapes: one mask block, a ragged last block, two blocks and a ragged tile, element loads, a second round of the four groups off 16-byte alignment,
the widest row, and a workgroup of the backward grid that walks on to a second row block.
"""
import itertools

import pytest
import torch

from fewbit_amd import cabi_x
from norm_harness import EPS, SEED, Guarded
from test_gpu_mx import DEV, DTYPES, defined, ids
from test_gpu_mx_glu import blocks
from test_gpu_norm import check_forward_values, inputs

pytestmark = pytest.mark.gpu
MASK_SEED = SEED + 4
WALKS_ON = 32 * cabi_x.MX_NORM_MAX_GRID + 33
# rows, width, strided (x, residual, gh and gy_add the column blocks of one buffer, one element off 16-byte alignment; width 13: p = 0 only)
CASES = [(1, 8, False), (31, 64, False), (33, 72, False), (65, 13, False), (65, 200, True), (33, 8192, False), (WALKS_ON, 8, False)]
every = pytest.mark.parametrize('dtype, format', [(d, f) for d in DTYPES[:2] for f in ('fp4', 'fp6')], ids=ids)
probabilities = lambda width: (0.0, 0.1, 1.0) if width % 8 == 0 else (0.0, )


@every
def test_forward_is_the_composition_bit_for_bit(dtype, format):
    for rows, width, strided in CASES:
        x, gamma, beta = inputs(rows, width, dtype)
        residual = inputs(rows, width, dtype, salt=1)[0]
        (xd, rd), _ = blocks(rows, width, dtype, strided, 2, (x, residual))
        gamma, beta = gamma.to(DEV), beta.to(DEV)
        seeds = torch.tensor([SEED, MASK_SEED], dtype=torch.int64, device=DEV)      # (device words, made once)
        for p, want_h in itertools.product(probabilities(width), (False, True)):
            b = None if (p, want_h) == (0.0, True) else beta                        # (once without beta)
            label = f'{rows} x {width} strided {strided} p {p} h {want_h}'
            h_ref = cabi_x.dropout_apply(xd.contiguous(), MASK_SEED, p, addend=rd.contiguous())
            y_ref, cells_ref, rstd_ref, mean_ref = cabi_x.mx_layer_norm_forward(h_ref, gamma, b, EPS, format, SEED)
            outs = [Guarded(rows * width, dtype), Guarded(rows * width, dtype), Guarded(rows, torch.float32), Guarded(cells_ref.numel(), torch.uint8),
                    Guarded(rows, torch.float32)]
            y, cells, rstd, h, mean = cabi_x.mx_add_layer_norm_forward(xd, rd, gamma, b, EPS, format, seeds if want_h else (SEED, MASK_SEED), p, want_h,
                                                                       outs[0].t.view(rows, width), outs[1].t.view(rows, width), outs[2].t, outs[3].t, outs[4].t)
            assert all(o.intact() for o in outs) and (want_h or outs[1].unchanged()), f'{label}: guard bytes, or an h that was not asked for'
            assert torch.equal(y, y_ref) and torch.equal(rstd, rstd_ref) and torch.equal(mean, mean_ref) and (h is None or torch.equal(h, h_ref)), label
            assert torch.equal(defined(cells, rows, width), defined(cells_ref, rows, width)), f'{label}: cells'
            if (rows, p, want_h) == (33, 0.1, True) and width == 72:                # once: the mask and the sum from the host, y and rstd against float64
                keep = cabi_x.dropout_keep(MASK_SEED, rows * width, p).view(rows, width)
                scale = torch.tensor(65536.0 / (65536 - cabi_x.dropout_threshold(p)), dtype=torch.float32)
                assert torch.equal(h.cpu(), torch.where(keep, (x.float() * scale + residual.float()).to(dtype), residual)), f'{label}: h'
                xhat = (h.cpu().float() - mean.cpu()[:, None]) * rstd.cpu()[:, None]
                check_forward_values(h.cpu(), gamma.cpu(), beta.cpu(), y.cpu(), rstd.cpu(), xhat, label)


@every
def test_backward_is_the_composition_bit_for_bit(dtype, format):
    for rows, width, strided in CASES:
        g = torch.Generator().manual_seed(7000 * width + rows)
        cells = cabi_x.mx_pack_host(torch.randn(rows, width, generator=g), SEED, format, 'kept').to(DEV)
        rstd = (0.25 + torch.rand(rows, generator=g)).to(DEV)
        gamma = (1 + 0.5 * torch.randn(width, generator=g)).to(dtype).to(DEV)
        (gy, gh, at_y), _ = blocks(rows, width, dtype, strided, 3, [torch.randn(rows, width, generator=g).to(dtype) for _ in range(3)])
        for arriving_y in (None, at_y):
            dx, dgamma_ref, dbeta_ref = cabi_x.mx_layer_norm_backward(gy.contiguous() if arriving_y is None else gy + arriving_y, cells, rstd, gamma, format)
            for p, arriving in itertools.product(probabilities(width)[:2], (None, gh)):
                dres_ref = dx if arriving is None else dx + arriving
                dbranch_ref = cabi_x.dropout_apply(dres_ref, MASK_SEED, p) if p else dres_ref
                for want in itertools.product((False, True), repeat=4):
                    label = f'{rows} x {width} strided {strided} p {p} gh {arriving is not None} gy_add {arriving_y is not None} want {want}'
                    got = cabi_x.mx_add_layer_norm_backward(gy, cells, rstd, gamma, format, MASK_SEED, p, arriving, want, arriving_y)
                    for name, out, ref, w in zip(('dres', 'dbranch', 'dgamma', 'dbeta'), got, (dres_ref, dbranch_ref, dgamma_ref, dbeta_ref), want):
                        assert (out is None and not w) or (w and torch.equal(out, ref)), f'{label}: {name}'
                    assert p or not (want[0] and want[1]) or got[0] is got[1], f'{label}: with p = 0 dres and dbranch are one tensor'


def test_what_is_refused_before_a_launch():
    x, gamma, beta = (t.to(DEV) for t in inputs(33, 13, torch.bfloat16))
    with pytest.raises(cabi_x.FewbitHipError, match='mx_add_layer_norm_forward.*multiple of 8'):
        cabi_x.mx_add_layer_norm_forward(x, x, gamma, beta, EPS, 'fp4', (SEED, MASK_SEED), 0.1)
    with pytest.raises(cabi_x.FewbitHipError, match='mx_add_layer_norm_forward: cells has'):
        cabi_x.mx_add_layer_norm_forward(x, x, gamma, beta, EPS, 'fp4', (SEED, MASK_SEED),
                                         cells=torch.empty(cabi_x.mx_bytes(33, 13, 'fp4') - 1, dtype=torch.uint8, device=DEV))
    y, rstd, cells = torch.empty_like(x), torch.empty(33, device=DEV), torch.empty(cabi_x.mx_bytes(33, 13, 'fp4'), dtype=torch.uint8, device=DEV)
    rc = cabi_x.lib().fewbit_hipx_mx_add_layer_norm_forward(cabi_x.DTYPES[x.dtype], x.data_ptr(), 13, None, 13, 33, 13, gamma.data_ptr(), None, EPS, 4, SEED,
                                                           MASK_SEED, None, 0, y.data_ptr(), 13, None, 0, None, rstd.data_ptr(), cells.data_ptr(), cells.numel(),
                                                           None)
    assert rc != 0 and 'mx_add_layer_norm_forward: null pointer (residual)' in cabi_x.lib().fewbit_hipx_last_error().decode()
