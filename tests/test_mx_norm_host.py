"""The normalized rows as row blocks without a GPU (include/fewbit_hipx.h; fewbit_amd/csrc/fewbit_mxnorm.hip): the three symbols, what the two entry
points refuse before anything is launched, the workspace, and ``fewbit.functional.rms_norm_linear_mx`` on host tensors: the outputs of the plain
composition, exact bias gradients, and a weight gradient whose mean over 200 seeds is ``G^T y`` (criterion 5 of EXPERIMENTS.md 8.32)."""
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi_x
from norm_harness import CALLS, worst_standard_error

NAMES = ('fewbit_hipx_mx_rms_norm_workspace', 'fewbit_hipx_mx_rms_norm_forward', 'fewbit_hipx_mx_rms_norm_backward')
P = 4096                                                                  # a pointer that is never followed: every call below is refused before a launch
CELLS, WORKSPACE = cabi_x.mx_bytes(40, 24, 'fp4'), 2 * 24 * 4
FORWARD = dict(dtype=2, x=P, ld_x=24, rows=40, width=24, gamma=P, eps=1e-5, format=4, seed=1, word=None, y=P, ld_y=24, rstd=P, cells=P, cells_bytes=CELLS, stream=None)
BACKWARD = dict(dtype=2, gy=P, ld_gy=24, cells=P, cells_bytes=CELLS, rstd=P, gamma=P, rows=40, width=24, format=4, dx=P, ld_dx=24, dgamma=P, workspace=P,
                workspace_bytes=WORKSPACE, stream=None)
REFUSALS = [('mx_rms_norm_forward', FORWARD, change, text) for change, text in (
    (dict(dtype=99), 'unknown dtype'), (dict(format=8), 'format'), (dict(format=5), 'format'), (dict(word=P + 4), 'seed word'), (dict(rows=0), 'rows'),
    (dict(width=0), 'width'), (dict(width=8193, ld_x=8193, ld_y=8193), 'width'), (dict(x=None), 'null'), (dict(gamma=None), 'null'), (dict(rstd=None), 'null'),
    (dict(ld_x=23), 'ld'), (dict(ld_y=23), 'ld'), (dict(y=P + 1), 'element'), (dict(cells=P + 8), '16-byte'), (dict(cells_bytes=CELLS - 1), 'bytes'))]
REFUSALS += [('mx_rms_norm_backward', BACKWARD, change, text) for change, text in (
    (dict(dtype=99), 'unknown dtype'), (dict(format=8), 'format'), (dict(width=0), 'width'), (dict(width=8193, ld_gy=8193, ld_dx=8193), 'width'),
    (dict(rows=2**30, width=8192, ld_gy=8192, ld_dx=8192), '2^36'), (dict(gy=None), 'null'), (dict(cells=None), 'null'), (dict(workspace=None), 'null'),
    (dict(ld_gy=23), 'ld'), (dict(ld_dx=23), 'ld'), (dict(dx=P + 1), 'element'), (dict(cells=P + 8), '16-byte'), (dict(cells_bytes=CELLS - 1), 'bytes'),
    (dict(workspace_bytes=WORKSPACE - 1), 'bytes'))]


@pytest.mark.parametrize('name, base, change, text', REFUSALS)
def test_what_the_entry_points_refuse_before_anything_is_launched(name, base, change, text):
    rc = getattr(cabi_x.lib(), 'fewbit_hipx_' + name)(*{**base, **change}.values())
    assert rc != 0 and text in cabi_x.lib().fewbit_hipx_last_error().decode()


def test_the_names_the_workspace_and_the_plan():
    root = Path(__file__).resolve().parent.parent
    header, exported = (root / 'include' / 'fewbit_hipx.h').read_text(), cabi_x.lib()
    assert all(name + '(' in header and name in cabi_x.SYMBOLS and hasattr(exported, name) for name in NAMES) and exported.fewbit_hipx_revision() == 2
    for rows, width in ((1, 8), (33, 72), (65, 200), (32 * cabi_x.MX_NORM_MAX_GRID + 1, 8), (2**20, 8192)):
        assert cabi_x.mx_rms_norm_workspace(rows, width) == min(-(-rows // 32), cabi_x.MX_NORM_MAX_GRID) * width * 4
    assert cabi_x.mx_rms_norm_workspace(0, 8) == cabi_x.mx_rms_norm_workspace(8, 0) == cabi_x.mx_rms_norm_workspace(8, cabi_x.MX_NORM_MAX_WIDTH + 1) == 0
    assert cabi_x.MX_NORM_PLAN_WIDTHS == () and cabi_x.MX_NORM_MAX_WIDTH == 8192               # one plan: x is read again at every width
    assert fewbit.MXNormLinear is fewbit.norm.MXNormLinear and fewbit.functional.rms_norm_linear_mx is fewbit.norm.rms_norm_linear_mx


@pytest.mark.parametrize('format', ('fp4', 'fp6'))
def test_the_node_on_host_tensors(format):
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(65, 64, generator=gen, requires_grad=True)
    gamma = (1 + 0.5 * torch.randn(64, generator=gen)).requires_grad_()
    weights = [(torch.randn(s, generator=gen) * 0.125).requires_grad_() for s in ((96, 64), (32, 64))]
    biases = [torch.randn(96, generator=gen).requires_grad_(), None]
    grads = [torch.randn(65, 96, generator=gen), torch.randn(65, 32, generator=gen)]
    y = F.rms_norm(x, (64, ), gamma, 1e-5)
    rounding = torch.Generator().manual_seed(11)
    samples = []
    for _ in range(CALLS):
        outs = fewbit.functional.rms_norm_linear_mx(x, gamma, weights, biases, 1e-5, format, rounding)
        d_weight, d_bias = torch.autograd.grad(outs, (weights[0], biases[0]), grads)
        samples.append(d_weight)
        assert torch.equal(d_bias, grads[0].sum(dim=0))
    assert outs[0].grad_fn.name() == '_RMSNormLinearMXBackward'
    for out, w, b in zip(outs, weights, biases):
        torch.testing.assert_close(out, F.linear(y, w, b), rtol=1e-5, atol=1e-5)
    worst = worst_standard_error(torch.stack(samples), (grads[0].T @ y).detach())
    print(f'{format}: the mean weight gradient of {CALLS} seeds is {worst:.2f} standard errors from G^T y in the worst entry')
    assert worst <= 5.0
    with pytest.raises(ValueError):
        fewbit.functional.rms_norm_linear_mx(x, gamma, weights, biases, format='fp8')
