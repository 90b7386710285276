"""``fewbit.functional.linear_mx`` / ``fewbit.MXLinear`` on the GPU (fewbit_amd/linear.py): everything but the weight gradient is ``F.linear``'s bits, the
weight gradient is ``cabi_x.mx_wgrad`` on the buffers of the recorded seed and unbiased over 200 seeds, an unserved width decodes and multiplies the
exact gradient, the node keeps ``mx_bytes`` and the weight, and a training step can be captured."""
import math

import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi, cabi_x, linear
from test_gpu_quant_linear import problem, saved_by, seeds  # noqa: F401  (the shapes are built exactly as there; `seeds` is its fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPE = (300, 64, 96)
BF16 = torch.bfloat16


@pytest.fixture(autouse=True)
def native_sketch_on():
    prev = linear.use_native_sketch(True)
    yield
    linear.use_native_sketch(prev)


def product(gy, x, seed, format):
    flat, g = x.detach().reshape(-1, x.shape[-1]), gy.reshape(-1, gy.shape[-1])
    return cabi_x.mx_wgrad(cabi_x.mx_pack(g, seed, 'fp8', 'grad'), cabi_x.mx_pack(flat, seed, format, 'kept'), flat.shape[0], flat.shape[1], g.shape[1], format)


@pytest.mark.parametrize('dtype', (BF16, torch.float16, torch.float32), ids=lambda d: str(d).split('.')[-1])
@pytest.mark.parametrize('format', ('fp4', 'fp6'))
def test_the_layer_against_f_linear_the_kernel_and_over_200_seeds(format, dtype, seeds):
    x, w, b, gy = problem(SHAPE, dtype)
    torch.manual_seed(0)
    yr = F.linear(x, w, b)
    gxr, gbr = torch.autograd.grad(yr, (x, b), gy)
    y, saved = saved_by(lambda: fewbit.functional.linear_mx(x, w, b, format))
    packed = [t for t in saved if t.dtype == torch.uint8]
    assert type(y.grad_fn).__name__ == '_LinearMXBackward' and len(seeds) == 1
    # saved for backward: mx_bytes of the input and the weight, nothing else
    assert len(saved) == 2 and len(packed) == 1 and packed[0].numel() == cabi_x.mx_bytes(SHAPE[0], SHAPE[1], format) and any(t.data_ptr() == w.data_ptr() for t in saved)
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), gy)
    assert torch.equal(y, yr) and torch.equal(gx, gxr) and torch.equal(gb, gbr)
    assert gw.dtype == w.dtype and torch.equal(gw, product(gy, x, seeds[0], format).to(w.dtype))
    if dtype != BF16:
        return
    exact, calls = gy.double().T @ x.detach().double(), 200
    total, squares = torch.zeros_like(exact), torch.zeros_like(exact)
    w32 = w.detach().float().requires_grad_()                              # (an fp32 weight: the mean is not taken over bf16 roundings of the sums)
    for _ in range(calls):
        (g, ) = torch.autograd.grad(fewbit.functional.linear_mx(x.detach().float(), w32, None, format), w32, gy.float())
        total += g.double()
        squares += g.double()**2
    mean = total / calls
    sd = (squares / calls - mean**2).clamp_min(0).sqrt() * math.sqrt(calls / (calls - 1))
    z = (mean - exact).abs() / (sd / math.sqrt(calls))
    print(f'{format}: worst entry {float(z.max()):.2f} standard errors; relative error of one call {float((g.double() - exact).norm() / exact.norm()):.4f}')
    assert len(set(seeds)) == 1 + calls and bool((sd > 0).all()) and float(z.max()) <= 5.0


def test_an_unserved_width_decodes_and_multiplies_the_exact_gradient(seeds):
    x, w, b, gy = problem((200, 72, 40), BF16)
    gw = torch.autograd.grad(fewbit.functional.linear_mx(x, w, b, 'fp6'), w, gy)[0]
    assert not cabi_x.mx_wgrad_serves(200, 72, 40, 'fp6')
    decoded = cabi_x.mx_unpack(cabi_x.mx_pack(x.detach(), seeds[0], 'fp6'), 200, 72, 'fp6', BF16)
    assert torch.equal(gw, gy.T @ decoded)
    assert torch.equal(decoded.cpu().float(), cabi_x.mx_unpack_host(cabi_x.mx_pack_host(x.detach().float().cpu(), seeds[0], 'fp6'), 200, 72, 'fp6').to(BF16).float())


def test_from_linear_under_map_module_shares_the_parameters_and_eval_keeps_nothing():
    model = torch.nn.Sequential(torch.nn.Linear(64, 96), torch.nn.GELU(), torch.nn.Linear(96, 32)).to(DEV, BF16)
    weights = [m.weight for m in model if isinstance(m, torch.nn.Linear)]
    mapped = fewbit.map_module(model, lambda m, path: fewbit.MXLinear.from_linear(m, 'fp6') if type(m) is torch.nn.Linear else m)
    layers = [m for m in mapped if isinstance(m, fewbit.MXLinear)]
    assert len(layers) == 2 and all(m.weight is w and m.format == 'fp6' for m, w in zip(layers, weights))
    x = torch.randn(8, 20, 64, device=DEV, dtype=BF16)
    y, saved = saved_by(lambda: mapped(x))
    assert sum(t.dtype == torch.uint8 for t in saved) == 2 and y.shape == (8, 20, 32)
    y.float().square().mean().backward()
    assert all(bool(m.weight.grad.isfinite().all()) for m in layers)
    assert not any(t.dtype == torch.uint8 for t in saved_by(lambda: mapped.eval()(x))[1])
    with torch.no_grad():
        assert saved_by(lambda: mapped.train()(x))[1] == []


def test_a_captured_training_step_replays_with_fresh_roundings(monkeypatch):
    x, w, b, gy = problem(SHAPE, BF16, 4)
    step = lambda: torch.autograd.grad(fewbit.functional.linear_mx(x, w, b, 'fp4'), (x, w), gy)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                        # the eager warm-up: the per-device replay counter exists from here on
    torch.cuda.current_stream().wait_stream(side)
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: 0x2468ace)
    counter = linear._replay_counter(torch.device(DEV))
    torch.cuda.synchronize()
    c0 = int(counter)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gx, gw = step()
    for replay in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gx, gy @ w.detach())
        assert torch.equal(gw, product(gy, x, cabi.mix_sketch_seed(0x2468ace, c0 + replay), 'fp4').to(BF16))
