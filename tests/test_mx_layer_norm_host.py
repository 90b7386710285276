"""The centred normalized rows as row blocks without a GPU (include/fewbit_hipx.h; fewbit_amd/csrc/fewbit_mxlnorm.hip): the three symbols, what the two
entry points refuse before anything is launched, the workspace, and ``fewbit.functional.layer_norm_linear_mx`` on host tensors: the outputs of the
plain composition, exact bias gradients, and a weight gradient whose mean over 200 seeds is ``G^T y`` with beta ~ N(0, 1) (criterion 5 of
EXPERIMENTS.md 8.32)."""
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi_x
from norm_harness import CALLS, worst_standard_error

NAMES = ('fewbit_hipx_mx_layer_norm_workspace', 'fewbit_hipx_mx_layer_norm_forward', 'fewbit_hipx_mx_layer_norm_backward')
P = 4096                                                                  # a pointer that is never followed: every call below is refused before a launch
CELLS, WORKSPACE = cabi_x.mx_bytes(40, 24, 'fp4'), 2 * 2 * 24 * 4
FORWARD = dict(dtype=2, x=P, ld_x=24, rows=40, width=24, gamma=P, beta=P, eps=1e-5, format=4, seed=1, word=None, y=P, ld_y=24, mean=P, rstd=P, cells=P,
               cells_bytes=CELLS, stream=None)
BACKWARD = dict(dtype=2, gy=P, ld_gy=24, cells=P, cells_bytes=CELLS, rstd=P, gamma=P, rows=40, width=24, format=4, dx=P, ld_dx=24, dgamma=P, dbeta=P,
                workspace=P, workspace_bytes=WORKSPACE, stream=None)
REFUSALS = [('mx_layer_norm_forward', FORWARD, change, text) for change, text in (
    (dict(dtype=99), 'unknown dtype'), (dict(format=8), 'format'), (dict(format=5), 'format'), (dict(word=P + 4), 'seed word'), (dict(rows=0), 'rows'),
    (dict(width=0), 'width'), (dict(width=8193, ld_x=8193, ld_y=8193), 'width'), (dict(x=None), 'null'), (dict(gamma=None), 'null'), (dict(rstd=None), 'null'),
    (dict(mean=None), 'null'), (dict(ld_x=23), 'ld'), (dict(ld_y=23), 'ld'), (dict(y=P + 1), 'element'), (dict(beta=P + 1), 'element'),
    (dict(cells=P + 8), '16-byte'), (dict(cells_bytes=CELLS - 1), 'bytes'),
    (dict(beta=None, cells_bytes=CELLS - 1), 'bytes'))]                      # beta may be null: the call gets as far as the size of the cells
REFUSALS += [('mx_layer_norm_backward', BACKWARD, change, text) for change, text in (
    (dict(dtype=99), 'unknown dtype'), (dict(format=8), 'format'), (dict(width=0), 'width'), (dict(width=8193, ld_gy=8193, ld_dx=8193), 'width'),
    (dict(rows=2**30, width=8192, ld_gy=8192, ld_dx=8192), '2^36'), (dict(gy=None), 'null'), (dict(cells=None), 'null'), (dict(workspace=None), 'null'),
    (dict(workspace=None, dgamma=None), 'null'), (dict(ld_gy=23), 'ld'), (dict(ld_dx=23), 'ld'), (dict(dx=P + 1), 'element'), (dict(dbeta=P + 2), 'element'),
    (dict(cells=P + 8), '16-byte'), (dict(cells_bytes=CELLS - 1), 'bytes'), (dict(workspace_bytes=WORKSPACE - 1), 'bytes'),
    (dict(workspace_bytes=WORKSPACE // 2, dgamma=None), 'bytes'))]           # dbeta alone takes the whole workspace: twice the RMS one


@pytest.mark.parametrize('name, base, change, text', REFUSALS)
def test_what_the_entry_points_refuse_before_anything_is_launched(name, base, change, text):
    rc = getattr(cabi_x.lib(), 'fewbit_hipx_' + name)(*{**base, **change}.values())
    assert rc != 0 and text in cabi_x.lib().fewbit_hipx_last_error().decode()


def test_the_names_and_the_workspace():
    root = Path(__file__).resolve().parent.parent
    header, exported = (root / 'include' / 'fewbit_hipx.h').read_text(), cabi_x.lib()
    assert all(name + '(' in header and name in cabi_x.SYMBOLS and hasattr(exported, name) for name in NAMES) and exported.fewbit_hipx_revision() == 2
    for rows, width in ((1, 8), (33, 72), (65, 200), (32 * cabi_x.MX_NORM_MAX_GRID + 1, 8), (2**20, 8192)):
        assert cabi_x.mx_layer_norm_workspace(rows, width) == min(-(-rows // 32), cabi_x.MX_NORM_MAX_GRID) * 2 * width * 4 == 2 * cabi_x.mx_rms_norm_workspace(rows, width)
    assert cabi_x.mx_layer_norm_workspace(0, 8) == cabi_x.mx_layer_norm_workspace(8, 0) == cabi_x.mx_layer_norm_workspace(8, cabi_x.MX_NORM_MAX_WIDTH + 1) == 0
    assert cabi_x.MX_NORM_PLAN_WIDTHS == ()                                    # one plan here as well: the row is read again at every width
    assert fewbit.MXLayerNormLinear is fewbit.norm.MXLayerNormLinear and fewbit.functional.layer_norm_linear_mx is fewbit.norm.layer_norm_linear_mx
    # nothing wanted: no launch, no workspace needed
    assert exported.fewbit_hipx_mx_layer_norm_backward(*{**BACKWARD, **dict(dx=None, dgamma=None, dbeta=None, workspace=None, workspace_bytes=0)}.values()) == 0


@pytest.mark.parametrize('format', ('fp4', 'fp6'))
def test_the_node_on_host_tensors(format):
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(65, 64, generator=gen, requires_grad=True)
    gamma, beta = (1 + 0.5 * torch.randn(64, generator=gen)).requires_grad_(), torch.randn(64, generator=gen).requires_grad_()
    weights = [(torch.randn(s, generator=gen) * 0.125).requires_grad_() for s in ((96, 64), (32, 64))]
    biases = [torch.randn(96, generator=gen).requires_grad_(), None]
    grads = [torch.randn(65, 96, generator=gen), torch.randn(65, 32, generator=gen)]
    y = F.layer_norm(x, (64, ), gamma, beta, 1e-5)
    rounding = torch.Generator().manual_seed(11)
    samples = []
    for _ in range(CALLS):
        outs = fewbit.functional.layer_norm_linear_mx(x, gamma, beta, weights, biases, 1e-5, format, rounding)
        d_weight, d_bias = torch.autograd.grad(outs, (weights[0], biases[0]), grads)
        samples.append(d_weight)
        assert torch.equal(d_bias, grads[0].sum(dim=0))
    assert outs[0].grad_fn.name() == '_LayerNormLinearMXBackward'
    for out, w, b in zip(outs, weights, biases):
        torch.testing.assert_close(out, F.linear(y, w, b), rtol=1e-5, atol=1e-5)
    worst = worst_standard_error(torch.stack(samples), (grads[0].T @ y).detach())
    print(f'{format}: the mean weight gradient of {CALLS} seeds is {worst:.2f} standard errors from G^T y in the worst entry')
    assert worst <= 5.0
    with pytest.raises(ValueError):
        fewbit.functional.layer_norm_linear_mx(x, gamma, beta, weights, biases, format='fp8')
