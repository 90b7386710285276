"""fewbit.QuantizedRMSNorm on the GPU: the layer on the kernels of fewbit_amd/csrc/fewbit_norm.hip.  The output is the RMS norm within the bound of
tests/test_gpu_rms_norm.py; what is saved is the state (``norm_state_bytes`` bytes), one fp32 rstd per row and gamma; the gradients are the
entry points' on the seed the call drew, bit for bit; and the layer inside checkpointing, autocast, no_grad / eval, a captured graph and with
the kernels switched off."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fewbit
import norm_harness as harness
from fewbit_amd import cabi_x, linear
from norm_harness import DEV, EPS, UNIT, native_sketch_on, saved_by, seeds  # noqa: F401 (the fixtures are used by name)

pytestmark = pytest.mark.gpu
KIND = harness.RMS_NORM
SHAPES = ((256, 64), (200, 72), (8, 25, 72))
DTYPES = (torch.bfloat16, torch.float32)
BITS = (2, 4, 8)
ids = lambda d: str(d).split('.')[-1] if isinstance(d, torch.dtype) else None


def problem(shape, dtype, salt=0):
    x, (w, ), gy = harness.problem(KIND, shape, dtype, salt)
    return x, w, gy


def entry_points(x, w, gy, bits, seed):
    """(y, dx, dgamma, state, rstd) of the entry points for `seed`"""
    y, grads, state, rstd = harness.entry_points(KIND, x, (w, ), gy, bits, seed)
    return (y, *grads, state, rstd)


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('dtype', DTYPES, ids=ids)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_the_layer_against_float64_and_the_recorded_seed(shape, dtype, bits, seeds):
    x, w, gy = problem(shape, dtype)
    width, rows = shape[-1], math.prod(shape[:-1])
    y, saved = saved_by(lambda: fewbit.functional.rms_norm_quantized(x, (width, ), w, EPS, bits))
    assert type(y.grad_fn).__name__ == '_RMSNormQuantizedBackward' and len(seeds) == 1 and y.shape == x.shape and y.dtype == dtype
    # y within the bound of the entry points' test: u |y| + K 2^-24 |x^| |gamma|, K = log2(width) + 4
    x64 = x.detach().double().cpu().reshape(rows, width)
    rstd64 = 1.0 / torch.sqrt(x64.square().mean(dim=1, keepdim=True) + float(np.float32(EPS)))
    xhat64 = x64 * rstd64
    y64 = xhat64 * w.detach().double().cpu()
    bound = UNIT[dtype] * y64.abs() + (math.log2(width) + 4) * 2.0**-24 * xhat64.abs() * w.detach().double().cpu().abs()
    assert bool(((y.detach().double().cpu().reshape(rows, width) - y64).abs() <= bound).all())
    theirs = float(((F.rms_norm(x.detach(), (width, ), w.detach(), EPS).double().cpu().reshape(rows, width) - y64).abs() / bound).max())
    print(f'{shape} {dtype} bits {bits}: F.rms_norm is at {theirs:.3f} of the bound of y')
    assert dtype != torch.float32 or theirs <= 1.0                    # (a 16-bit F.rms_norm may round x^ before the weight)
    # saved: exactly the state, rstd and gamma
    assert len(saved) == 3 and saved[0].dtype == torch.uint8 and saved[0].numel() == cabi_x.norm_state_bytes(rows, width, bits)
    assert saved[1].dtype == torch.float32 and saved[1].numel() == rows and (saved[2] is w or saved[2].data_ptr() == w.data_ptr())
    assert saved[0].numel() + 4 * saved[1].numel() == cabi_x.norm_state_bytes(rows, width, bits) + 4 * rows
    # the gradients are the entry points' on the recorded seed, bit for bit
    gx, gw = torch.autograd.grad(y, (x, w), gy)
    ye, dxe, dge, state, rstd = entry_points(x, w, gy, bits, seeds[0])
    assert torch.equal(y, ye) and torch.equal(saved[0], state) and torch.equal(saved[1], rstd)
    assert gx.dtype == gw.dtype == dtype and gx.shape == x.shape
    assert torch.equal(gx, dxe) and torch.equal(gw, dge.to(dtype))
    # and the state is the host's for that seed, from the float64 x^ within the step of each group (one code either way at a border)
    decoded = cabi_x.norm_state_unpack_host(state.cpu(), rows, width, bits).double()
    step = state.cpu()[:8 * rows * math.ceil(width / 64)].view(torch.float32).view(rows, -1, 2)[:, :, 1].double().repeat_interleave(64, dim=1)[:, :width]
    assert bool(((decoded - xhat64).abs() <= step * (1 + 1e-5) + 1e-5).all())


@pytest.mark.parametrize('reentrant', (False, True))
def test_checkpointing_gives_the_plain_runs_bits(reentrant):
    harness.checkpointing_gives_the_plain_runs_bits(KIND, SHAPES[1], reentrant)


def test_backward_may_follow_the_autocast_block(seeds):
    harness.backward_may_follow_the_autocast_block(KIND, SHAPES[1], seeds)


def test_no_grad_eval_and_frozen_parameters_build_no_node_and_keep_no_state(seeds):
    x, w, gy = problem(SHAPES[1], torch.bfloat16, 3)
    harness.no_grad_eval_and_frozen_parameters_build_no_node_and_keep_no_state(KIND, x, seeds)
    # eps=None on the kernels: torch.finfo(input.dtype).eps
    none = fewbit.QuantizedRMSNorm(x.shape[-1], device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        flat = x.detach()
        assert torch.equal(none(x), cabi_x.rms_norm_forward(flat, none.weight.detach(), torch.finfo(torch.bfloat16).eps, keep=False)[0])
    harness.a_non_contiguous_input_is_normalized_from_a_contiguous_copy(KIND, x, (w, ), gy, seeds)


def test_with_the_kernels_switched_off_the_host_formulation_runs_on_the_gpu_tensor():
    x, w, gy = problem(SHAPES[1], torch.bfloat16, 5)
    rows, width = SHAPES[1]
    prev = linear.use_native_sketch(False)
    try:
        y, saved = saved_by(lambda: fewbit.functional.rms_norm_quantized(x, (width, ), w, EPS, 4))
        gx, gw = torch.autograd.grad(y, (x, w), gy)
    finally:
        linear.use_native_sketch(prev)
    # codes one per byte of the rows padded to whole groups, lo, step, rstd, gamma; y is F.rms_norm's
    assert len(saved) == 5 and saved[0].numel() == rows * 128 and saved[0].device.type == 'cuda' and torch.equal(y, F.rms_norm(x, (width, ), w, EPS))
    codes, lo, step, rstd, _ = saved
    xq = torch.addcmul(lo.double()[:, None], codes.view(-1, 64).double(), step.double()[:, None]).view(rows, -1)[:, :width]
    gh = gy.double() * w.detach().double()
    dx = rstd.double()[:, None] * (gh - xq * (gh * xq).mean(dim=1, keepdim=True))
    assert gx.dtype == gw.dtype == torch.bfloat16
    assert bool(((gx.double() - dx).abs() <= (2.0**-8 + 1e-5) * rstd.double()[:, None] * (gh.abs() + xq.abs() * (gh * xq).abs().mean(dim=1, keepdim=True))).all())
    assert bool(((gw.double() - (gy.double() * xq).sum(dim=0)).abs() <= (2.0**-8 + 1e-5) * (gy.double() * xq).abs().sum(dim=0)).all())
    # float64 and rows wider than the kernels' take it too
    wide = torch.randn(2, 8200, device=DEV, requires_grad=True)
    y, saved = saved_by(lambda: fewbit.functional.rms_norm_quantized(wide, (8200, ), bits=4))
    assert len(saved) == 4 and saved[0].numel() == 2 * 8256
    torch.autograd.grad(y, wide, torch.ones_like(y))


def test_a_captured_step_rounds_afresh_on_every_replay(monkeypatch):
    harness.a_captured_step_rounds_afresh_on_every_replay(KIND, SHAPES[0], monkeypatch)
