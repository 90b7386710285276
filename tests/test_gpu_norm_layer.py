"""fewbit.QuantizedLayerNorm on the GPU: the layer on the kernels of fewbit_amd/csrc/fewbit_norm.hip.  The output is the layer norm within the
bound of tests/test_gpu_norm.py; what is saved is the state (``norm_state_bytes`` bytes), one fp32 rstd per row and gamma; the gradients are
the entry points' on the seed the call drew, bit for bit; over 200 calls the weight gradient is unbiased and the input gradient averages out
up to its second-order bias (the two statistics of tests/test_norm_host.py, on the kernels, in fp32); and the layer inside checkpointing,
autocast, no_grad / eval and a captured graph."""
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
KIND = harness.LAYER_NORM
SHAPES = ((256, 64), (200, 72), (8, 25, 72))
DTYPES = (torch.bfloat16, torch.float32)
BITS = (2, 4, 8)
ids = lambda d: str(d).split('.')[-1] if isinstance(d, torch.dtype) else None


def problem(shape, dtype, salt=0):
    x, (w, b), gy = harness.problem(KIND, shape, dtype, salt)
    return x, w, b, gy


def entry_points(x, w, b, gy, bits, seed):
    """(y, dx, dgamma, dbeta, state, rstd) of the entry points for `seed`"""
    y, grads, state, rstd = harness.entry_points(KIND, x, (w, b), gy, bits, seed)
    return (y, *grads, state, rstd)


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('dtype', DTYPES, ids=ids)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_the_layer_against_f_layer_norm_and_the_recorded_seed(shape, dtype, bits, seeds):
    x, w, b, gy = problem(shape, dtype)
    width, rows = shape[-1], math.prod(shape[:-1])
    y, saved = saved_by(lambda: fewbit.functional.layer_norm_quantized(x, (width, ), w, b, EPS, bits))
    assert type(y.grad_fn).__name__ == '_LayerNormQuantizedBackward' and len(seeds) == 1 and y.shape == x.shape and y.dtype == dtype
    # y within the bound of the entry points' test: u |y| + K 2^-24 (|x^| + |mean| rstd + 1) |gamma| + 2^-24 |beta|, K = log2(width) + 4
    x64 = x.detach().double().cpu().reshape(rows, width)
    mean = x64.mean(dim=1, keepdim=True)
    rstd64 = 1.0 / torch.sqrt((x64 - mean).square().mean(dim=1, keepdim=True) + float(np.float32(EPS)))
    xhat64 = (x64 - mean) * rstd64
    y64 = xhat64 * w.detach().double().cpu() + b.detach().double().cpu()
    bound = (UNIT[dtype] * y64.abs() + (math.log2(width) + 4) * 2.0**-24 * (xhat64.abs() + mean.abs() * rstd64 + 1) * w.detach().double().cpu().abs()
             + 2.0**-24 * b.detach().double().cpu().abs())
    assert bool(((y.detach().double().cpu().reshape(rows, width) - y64).abs() <= bound).all())
    assert bool(((F.layer_norm(x.detach(), (width, ), w.detach(), b.detach(), EPS).double().cpu().reshape(rows, width) - y64).abs() <= bound).all())
    # saved: exactly the state, rstd and gamma
    assert len(saved) == 3 and saved[0].dtype == torch.uint8 and saved[0].numel() == cabi_x.norm_state_bytes(rows, width, bits)
    assert saved[1].dtype == torch.float32 and saved[1].numel() == rows and (saved[2] is w or saved[2].data_ptr() == w.data_ptr())
    # the gradients are the entry points' on the recorded seed, bit for bit
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), gy)
    ye, dxe, dge, dbe, state, rstd = entry_points(x, w, b, gy, bits, seeds[0])
    assert torch.equal(y, ye) and torch.equal(saved[0], state) and torch.equal(saved[1], rstd)
    assert gx.dtype == gw.dtype == gb.dtype == dtype and gx.shape == x.shape
    assert torch.equal(gx, dxe) and torch.equal(gw, dge.to(dtype)) and torch.equal(gb, dbe.to(dtype))
    # and the state is the host's for that seed, from the float64 x^ within the step of each group (one code either way at a border)
    decoded = cabi_x.norm_state_unpack_host(state.cpu(), rows, width, bits).double()
    step = state.cpu()[:8 * rows * math.ceil(width / 64)].view(torch.float32).view(rows, -1, 2)[:, :, 1].double().repeat_interleave(64, dim=1)[:, :width]
    assert bool(((decoded - xhat64).abs() <= step * (1 + 1e-5) + 1e-5).all())


CALLS = 200


def gradients_over_calls(bits):
    rows, width = 48, 200
    x, w, b, gy = problem((rows, width), torch.float32, 9)
    x64 = x.detach().double()
    centred = x64 - x64.mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(centred.square().mean(dim=1, keepdim=True) + EPS)
    xhat, gh = centred * rstd, gy.double() * w.detach().double()
    dx = rstd * (gh - gh.mean(dim=1, keepdim=True) - xhat * (gh * xhat).mean(dim=1, keepdim=True))
    dgamma = (gy.double() * xhat).sum(dim=0)
    layer = fewbit.QuantizedLayerNorm(width, eps=EPS, bits=bits, device=DEV)
    with torch.no_grad():
        layer.weight.copy_(w)
        layer.bias.copy_(b)
    torch.manual_seed(0)
    dxs, dgs = [], []
    for _ in range(CALLS):
        gx, gw = torch.autograd.grad(layer(x), (x, layer.weight), gy)
        dxs.append(gx.double())
        dgs.append(gw.double())
    return dx, dgamma, torch.stack(dxs), torch.stack(dgs)


@pytest.mark.parametrize('bits', BITS)
def test_the_statistics_of_the_definition_on_the_kernels(bits, seeds):
    """fp32 only: in bf16 at 8 bits the rounding of the output exceeds the quantization noise, and R would measure that instead"""
    dx, dgamma, dxs, dgs = gradients_over_calls(bits)
    assert len(seeds) == CALLS and len(set(seeds)) == CALLS
    sd = dgs.std(dim=0)
    z = float(((dgs.mean(dim=0) - dgamma).abs() / (sd / math.sqrt(CALLS))).max())
    one_call = math.sqrt(float((dxs - dx).square().sum(dim=(1, 2)).mean()))
    R = float((dxs.mean(dim=0) - dx).norm()) / (one_call / math.sqrt(CALLS))
    print(f'bits {bits}: worst entry of dgamma {z:.2f} standard errors; R = {R:.3f}, relative error of one call {one_call / float(dx.norm()):.5f}')
    assert bool((sd > 0).all()) and z <= 5.0
    assert R <= 1.5


@pytest.mark.parametrize('reentrant', (False, True))
def test_checkpointing_gives_the_plain_runs_bits(reentrant):
    harness.checkpointing_gives_the_plain_runs_bits(KIND, SHAPES[1], reentrant)


def test_backward_may_follow_the_autocast_block(seeds):
    x16, (w, b) = harness.backward_may_follow_the_autocast_block(KIND, SHAPES[1], seeds)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        assert F.layer_norm(x16, (x16.shape[-1], ), w, b, EPS).dtype == torch.float32        # (what torch does there)


def test_no_grad_eval_and_frozen_parameters_build_no_node_and_keep_no_state(seeds):
    x, w, b, gy = problem(SHAPES[1], torch.bfloat16, 3)
    harness.no_grad_eval_and_frozen_parameters_build_no_node_and_keep_no_state(KIND, x, seeds)
    # the switch, float64 and rows wider than the kernels': the PyTorch formulation (codes one per byte)
    prev = linear.use_native_sketch(False)
    try:
        y, saved = saved_by(lambda: fewbit.functional.layer_norm_quantized(x, (x.shape[-1], ), w, b, EPS, 4))
    finally:
        linear.use_native_sketch(prev)
    assert len(saved) == 5 and saved[0].numel() == x.shape[0] * 128 and torch.equal(y, F.layer_norm(x, (x.shape[-1], ), w, b, EPS))
    wide = torch.randn(2, 8200, device=DEV, requires_grad=True)
    y, saved = saved_by(lambda: fewbit.functional.layer_norm_quantized(wide, (8200, ), bits=4))
    assert len(saved) == 4 and saved[0].numel() == 2 * 8256
    torch.autograd.grad(y, wide, torch.ones_like(y))
    harness.a_non_contiguous_input_is_normalized_from_a_contiguous_copy(KIND, x, (w, b), gy, seeds)


def test_a_captured_step_rounds_afresh_on_every_replay(monkeypatch):
    harness.a_captured_step_rounds_afresh_on_every_replay(KIND, SHAPES[0], monkeypatch)
