"""The two kernels of fewbit_amd/csrc/fewbit_mxlnorm.hip (cabi_x.mx_layer_norm_forward / mx_layer_norm_backward) against their definition
(include/fewbit_hipx.h, "The centred normalized rows as row blocks"): mean, rstd, y and dx within the bounds of the existing layer norm
(test_gpu_norm.py: twice what plain fp32 torch ops measure in the same call, floor log2 width + 4); given the mean and the rstd the kernel wrote, y and
the cells bit for bit from host fp32 arithmetic and mx_pack_host.
"""
import pytest
import torch

from fewbit_amd import cabi_x
from norm_harness import EPS, SEED
from test_gpu_mx import DEV, DTYPES, defined, ids
from test_gpu_mx_glu import blocks
from test_gpu_norm import check_backward_values, check_forward_values, inputs

pytestmark = pytest.mark.gpu
WALKS_ON = 32 * cabi_x.MX_NORM_MAX_GRID + 33                                    # rows: one row block more than the backward grid has workgroups
# rows, width, strided (every tensor a column block of one buffer, one element off 16-byte alignment)
CASES = ([(1, 8, False), (31, 64, False), (33, 72, False), (65, 200, False), (33, 72, True), (33, 8192, False), (WALKS_ON, 8, False)]
         + [(33, w + d, False) for w in cabi_x.MX_NORM_PLAN_WIDTHS for d in (0, 8)])
every = pytest.mark.parametrize('dtype, format', [(d, f) for d in DTYPES for f in ('fp4', 'fp6')], ids=ids)


def forward(x, gamma, beta, format, seed, strided=False):
    """-> (y, cells, rstd, mean) on the host, after the gaps of the strided buffer were checked"""
    (xd, yd), gaps = blocks(*x.shape, x.dtype, strided, 2, (x, ))
    outs = cabi_x.mx_layer_norm_forward(xd, gamma.to(DEV), None if beta is None else beta.to(DEV), EPS, format, seed, y=yd)
    assert gaps is None or bool((gaps == 7).all()), 'the gaps between the column blocks were written'
    return tuple(t.cpu() for t in outs)


def definition(x, gamma, beta, mean, rstd):
    """(x^, y) of host fp32 arithmetic from the kernel's own mean and rstd"""
    xhat = (x.float() - mean[:, None]) * rstd[:, None]
    y = xhat * gamma.float()
    return xhat, (y if beta is None else y + beta.float()).to(x.dtype)


@every
def test_forward_is_the_definition_bit_for_bit_from_its_own_statistics(dtype, format):
    for i, (rows, width, strided) in enumerate(CASES):
        label = f'{rows} x {width} strided {strided}'
        x, gamma, beta = inputs(rows, width, dtype)
        y, cells, rstd, mean = forward(x, gamma, beta, format, SEED, strided)
        if i == 2:                                                              # one case without beta: the same statistics and cells, nothing is added
            bare = forward(x, gamma, None, format, SEED, strided)
            assert torch.equal(bare[0], definition(x, gamma, None, mean, rstd)[1]) and torch.equal(bare[2], rstd) and torch.equal(bare[3], mean), label
            assert torch.equal(defined(bare[1], rows, width), defined(cells, rows, width)), label
        xhat, want_y = definition(x, gamma, beta, mean, rstd)
        check_forward_values(x, gamma, beta, y, rstd, xhat, label)
        assert torch.equal(y, want_y), f'{label}: y'
        want, got = defined(cabi_x.mx_pack_host(xhat, SEED, format, 'kept'), rows, width), defined(cells, rows, width)
        assert torch.equal(got, want), f'{label}: cells differ at bytes {torch.nonzero(got != want).flatten()[:8].tolist()}'
        word = torch.tensor([SEED], dtype=torch.int64, device=DEV)
        for seed in (word, SEED):                                               # the seed as a device word; the same call twice
            again = forward(x, gamma, beta, format, seed, strided)
            assert torch.equal(again[0], y) and torch.equal(defined(again[1], rows, width), got) and torch.equal(again[2], rstd) and torch.equal(again[3], mean), label


@every
def test_a_constant_row_block_is_beta_with_scale_bytes_0_and_codes_0(dtype, format):
    rows, width = 65, 72
    x, gamma, beta = inputs(rows, width, dtype)
    x[32:64] = torch.arange(32, dtype=torch.float32).to(dtype)[:, None]          # every row of block 1 constant (a value of its own, exact in bf16)
    y, cells, rstd, mean = forward(x, gamma, beta, format, SEED)
    assert torch.equal(y[32:64], beta.expand(32, width)) and torch.equal(y, definition(x, gamma, beta, mean, rstd)[1])
    scales, codes = cells[:3 * width].view(3, width), cells[-(-3 * width // 16) * 16:].view(3, -1)
    assert bool((scales[1] == 0).all()) and bool((codes[1] == 0).all()) and bool((scales[0] != 0).all()) and bool((codes[2] != 0).any())


@every
def test_backward_from_a_given_state(dtype, format):
    for i, (rows, width, strided) in enumerate(CASES):
        label = f'{rows} x {width} strided {strided}'
        g = torch.Generator().manual_seed(7000 * width + rows)
        cells = cabi_x.mx_pack_host(torch.randn(rows, width, generator=g), SEED, format, 'kept')
        xq = cabi_x.mx_unpack_host(cells, rows, width, format)
        rstd = 0.25 + torch.rand(rows, generator=g)
        gy = torch.randn(rows, width, generator=g).to(dtype)
        gamma = (1 + 0.5 * torch.randn(width, generator=g)).to(dtype)
        (gyd, dxd), gaps = blocks(rows, width, dtype, strided, 2, (gy, ))
        state = (cells.to(DEV), rstd.to(DEV), gamma.to(DEV), format)
        dx, dgamma, dbeta = cabi_x.mx_layer_norm_backward(gyd, *state, dx=dxd)
        check_backward_values(xq, rstd, gy, gamma, dx.cpu(), dgamma.cpu(), dbeta.cpu(), label)
        assert gaps is None or bool((gaps == 7).all()), f'{label}: the gaps between the column blocks were written'
        if i == 3:                                                              # what is not wanted is not written, what is keeps its bytes
            full = (dx, dgamma, dbeta)
            for want in ((True, False, False), (False, True, False), (False, False, True), (False, True, True)):
                got = cabi_x.mx_layer_norm_backward(gyd, *state, want=want)
                assert all((out is None and not w) or (w and torch.equal(out, ref)) for out, ref, w in zip(got, full, want)), (label, want)


@every
def test_one_nan_poisons_its_row_its_cells_and_nothing_else(dtype, format):
    rows, width, at = 65, 72, 40
    x, gamma, beta = inputs(rows, width, dtype)
    clean = forward(x, gamma, beta, format, SEED)[0]
    x[at, 5] = float('nan')
    y, cells, rstd, mean = forward(x, gamma, beta, format, SEED)
    others = torch.arange(rows) != at
    assert bool(y[at].isnan().all()) and torch.equal(y[others], clean[others])
    assert bool((cells[:3 * width].view(3, width) == 0xFF).all(dim=1).tolist() == [False, True, False])
    gy = torch.ones(rows, width, dtype=dtype, device=DEV)
    dx, dgamma, dbeta = cabi_x.mx_layer_norm_backward(gy, cells.to(DEV), torch.ones(rows, device=DEV), gamma.to(DEV), format)
    block = (torch.arange(rows) // 32 == at // 32).to(DEV)
    assert bool(dx[block].isnan().all()) and bool(dx[~block].isfinite().all()) and bool(dgamma.isnan().all()) and bool(dbeta.isfinite().all())
