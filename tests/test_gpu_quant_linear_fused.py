"""The quantized layers with ``linear.use_fused_weight_gradient(True)``: the weight gradient is ``cabi_x.quant_wgrad`` on the buffer the layer kept -- the
MFMA kernel that decodes the codes on their way into the matrix pipe (fewbit_amd/csrc/fewbit_qgemm.hip) -- everything else is what it was, a call
the kernel does not serve gives the bits of the default route, and backward allocates nothing of the input's size."""
import math

import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi, cabi_x, glu, linear
from test_gpu_quant_linear import problem, saved_by, seeds  # noqa: F401  (the shape is built exactly as there; `seeds` is its fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPE = (256, 64, 32)
BF16 = torch.bfloat16


@pytest.fixture(autouse=True)
def fused_on():
    prev = linear.use_native_sketch(True), linear.use_fused_weight_gradient(True)
    yield
    linear.use_native_sketch(prev[0])
    linear.use_fused_weight_gradient(prev[1])


def fused(gy, x, seed, bits):
    flat = x.detach().reshape(-1, x.shape[-1]).contiguous()
    return cabi_x.quant_wgrad(gy.reshape(-1, gy.shape[-1]), cabi_x.quant_pack(flat, seed, bits), flat.shape[1], bits, torch.float32)


@pytest.mark.parametrize('bits', (2, 4, 8))
def test_the_layer_against_f_linear_the_kernel_and_over_200_seeds(bits, seeds):
    """bf16 at 8 bits, 200 seeds: the operand values are those of the two-term route, which sits 3.80 standard errors off at this shape and seed stream
    (EXPERIMENTS.md 8.17); the criterion is the project's own, 5."""
    x, w, b, gy = problem(SHAPE, BF16)
    torch.manual_seed(0)
    yr = F.linear(x, w, b)
    gxr, gbr = torch.autograd.grad(yr, (x, b), gy)
    y, saved = saved_by(lambda: fewbit.functional.linear_quantized(x, w, b, bits))
    packed = [t for t in saved if t.dtype == torch.uint8]
    assert len(saved) == 2 and len(packed) == 1 and any(t.data_ptr() == w.data_ptr() for t in saved)
    before = packed[0].clone(), w.detach().clone()
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), gy)
    assert torch.equal(y, yr) and torch.equal(gx, gxr) and torch.equal(gb, gbr)
    assert gw.dtype == w.dtype and torch.equal(gw, fused(gy, x, seeds[0], bits).to(w.dtype))
    assert torch.equal(packed[0], before[0]) and torch.equal(packed[0].cpu(), cabi_x.quant_pack_host(x.detach().float().cpu(), seeds[0], bits)) and torch.equal(w, before[1])
    if bits != 8:
        return
    exact, calls = gy.double().T @ x.detach().double(), 200
    total, squares = torch.zeros_like(exact), torch.zeros_like(exact)
    layer = fewbit.QuantizedLinear(SHAPE[1], SHAPE[2], bits=bits, device=DEV, dtype=BF16)
    with torch.no_grad():
        layer.weight.copy_(w)
        layer.bias.copy_(b)
    for _ in range(calls):
        (g, ) = torch.autograd.grad(layer(x), layer.weight, gy)
        total += g.double()
        squares += g.double()**2
    mean = total / calls
    sd = (squares / calls - mean**2).clamp_min(0).sqrt() * math.sqrt(calls / (calls - 1))
    z = (mean - exact).abs() / (sd / math.sqrt(calls))
    print(f'bf16, 8 bits, fused: worst entry {float(z.max()):.2f} standard errors')
    assert len(set(seeds)) == 1 + calls and bool((sd > 0).all()) and float(z.max()) <= 5.0


@pytest.mark.parametrize('shape, dtype', (((200, 72, 40), BF16), (SHAPE, torch.float32)), ids=('in72', 'fp32'))
def test_a_call_the_kernel_does_not_serve_gives_the_default_routes_bits(shape, dtype):
    x, w, b, gy = problem(shape, dtype)
    got = []
    for on in (False, True):
        linear.use_fused_weight_gradient(on)
        torch.manual_seed(3)
        got.append(torch.autograd.grad(fewbit.functional.linear_quantized(x, w, b, 8), (x, w, b), gy))
    assert all(torch.equal(a, c) for a, c in zip(*got))


def test_the_gated_mlp_forms_both_projection_gradients_on_the_kernel(monkeypatch):
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(96, 64, generator=gen).to(BF16).to(DEV).requires_grad_()
    wg, wu, wd = ((torch.randn(shape, generator=gen) / 8).to(BF16).to(DEV).requires_grad_() for shape in ((128, 64), (128, 64), (64, 128)))
    gy = torch.randn(96, 64, generator=gen).to(BF16).to(DEV)
    calls, real = [], cabi_x.quant_wgrad
    monkeypatch.setattr(cabi_x, 'quant_wgrad', lambda g, packed, *rest: calls.append((g.clone(), packed.clone(), rest)) or real(g, packed, *rest))
    got = []
    for on in (False, True):
        linear.use_fused_weight_gradient(on)
        torch.manual_seed(4)
        got.append(torch.autograd.grad(glu.gated_mlp_quantized(x, wg, wu, wd, bits=4), (x, wg, wu, wd), gy))
    (dx0, dg0, du0, dd0), (dx1, dg1, du1, dd1) = got
    assert torch.equal(dx0, dx1) and torch.equal(dd0, dd1) and len(calls) == 2
    for (g, packed, rest), on, off in zip(calls, (dg1, du1), (dg0, du0)):
        assert rest == (64, 4, torch.float32) and packed.numel() == cabi_x.quant_bytes(96 * 64, 4)
        assert torch.equal(on, real(g, packed, *rest).to(BF16))
        assert bool(((on.float() - off.float()).abs() <= 2.0**-7 * off.float().abs() + 1e-30).all())          # the same operands: one bf16 step at the most


def test_backward_allocates_nothing_of_the_inputs_size():
    rows, fin, fout = 8192, 1024, 64
    x = torch.randn(rows, fin, device=DEV, dtype=BF16)
    w = torch.randn(fout, fin, device=DEV, dtype=BF16, requires_grad=True)
    gy = torch.randn(rows, fout, device=DEV, dtype=BF16)
    peak = []
    for on in (True, False):
        linear.use_fused_weight_gradient(on)
        y = fewbit.functional.linear_quantized(x, w, None, 4)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        torch.autograd.grad(y, w, gy)
        torch.cuda.synchronize()
        peak.append(torch.cuda.max_memory_allocated() - before)
    print(f'peak over backward: fused {peak[0]} bytes, default {peak[1]} bytes; the decode is {rows * fin * 2}')
    assert peak[0] < rows * fin * 2 <= peak[1]


def test_a_captured_step_replays_with_the_switch_on(monkeypatch):
    x, w, b, gy = problem(SHAPE, BF16, 4)
    step = lambda: torch.autograd.grad(fewbit.functional.linear_quantized(x, w, b, 8), (x, w), gy)
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
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gx, gy @ w.detach())
        assert torch.equal(gw, fused(gy, x, cabi.mix_sketch_seed(0x2468ace, c0 + replay), 8).to(BF16))
