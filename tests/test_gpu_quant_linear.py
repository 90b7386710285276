"""fewbit.QuantizedLinear on the GPU: the layer on the kernels of fewbit_amd/csrc/fewbit_quant.hip.  The output and the input gradient are
``F.linear``'s bit for bit; the weight gradient is ``G^T quant_unpack(quant_pack(X, seed))`` for the seed the call drew, and over 200 seeds
within 5 standard errors of the exact one; what is saved of the input is ``quant_bytes(N, bits)`` bytes."""
import math

import pytest
import torch
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

import fewbit
from fewbit_amd import cabi, cabi_x, linear

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = ((256, 64, 32), (200, 72, 40))                               # rows, in_features, out_features
DTYPES = (torch.bfloat16, torch.float32)
BITS = (2, 4, 8)
ids = lambda d: str(d).split('.')[-1] if isinstance(d, torch.dtype) else None


@pytest.fixture(autouse=True)
def native_sketch_on():
    prev = linear.use_native_sketch(True)
    yield
    linear.use_native_sketch(prev)


@pytest.fixture
def seeds(monkeypatch):
    """the seeds the layer draws, in order"""
    drawn = []
    real = linear._draw_seed

    def draw(generator):
        drawn.append(real(generator))
        return drawn[-1]

    monkeypatch.setattr(linear, '_draw_seed', draw)
    return drawn


def saved_by(call):
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        result = call()
    return result, saved


def problem(shape, dtype, salt=0):
    rows, fin, fout = shape
    g = torch.Generator().manual_seed(31 + salt)
    x = torch.randn(rows, fin, generator=g).to(dtype).to(DEV).requires_grad_()
    w = (torch.randn(fout, fin, generator=g) / math.sqrt(fin)).to(dtype).to(DEV).requires_grad_()
    b = torch.randn(fout, generator=g).to(dtype).to(DEV).requires_grad_()
    gy = torch.randn(rows, fout, generator=g).to(dtype).to(DEV)
    return x, w, b, gy


def decoded_by(x, seed, bits, dtype):
    """quant_unpack(quant_pack(X, seed)) in `dtype`, as a matrix"""
    flat = x.detach().reshape(-1, x.shape[-1]).contiguous()
    return cabi_x.quant_unpack(cabi_x.quant_pack(flat, seed, bits), flat.numel(), bits, dtype).view(flat.shape)


def weight_gradient_by(gy, x, seed, bits, dtype):
    """G^T quant_unpack(quant_pack(X, seed)) as the layer forms it: the decode in the gradient's dtype and one GEMM; for a bf16 gradient at 8
    bits the fp32 decode as its bf16 rounding and the bf16 rounding of the exact remainder, two GEMMs with fp32 results, summed (fp32)"""
    g = gy.reshape(-1, gy.shape[-1])
    if bits == 8 and dtype == torch.bfloat16:
        decoded = decoded_by(x, seed, bits, torch.float32)
        head = decoded.bfloat16()
        assert torch.equal(head.view(torch.int16), decoded_by(x, seed, bits, dtype).view(torch.int16))
        tail = (decoded - head.float()).bfloat16()
        return torch.mm(g.T, head, out_dtype=torch.float32) + torch.mm(g.T, tail, out_dtype=torch.float32)
    return g.T @ decoded_by(x, seed, bits, dtype)


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('dtype', DTYPES, ids=ids)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_the_layer_against_f_linear_and_the_recorded_seed(shape, dtype, bits, seeds):
    """The last assertion is what ``linear._decode_in_two_terms`` is for: with X^ decoded into bf16 at 8 bits the worst entry of the mean over
    these 200 seeds was 8.49 and 8.63 standard errors off at the two shapes (every other case 3.2 - 4.4) -- rounding ``lo + code * step`` to
    bf16 moves an element by up to half a bf16 ulp whatever the seed, and at 8 bits the step is about one ulp."""
    x, w, b, gy = problem(shape, dtype)
    torch.manual_seed(0)                                              # the 201 seeds of this test: the same in every run
    yr = F.linear(x, w, b)
    gxr, gwr, gbr = torch.autograd.grad(yr, (x, w, b), gy)
    y, saved = saved_by(lambda: fewbit.functional.linear_quantized(x, w, b, bits))
    assert type(y.grad_fn).__name__ == '_LinearQuantizedBackward' and len(seeds) == 1
    assert torch.equal(y, yr)
    # saved: the packed buffer and the weight -- of the input, quant_bytes(N, bits) bytes
    packed = [t for t in saved if t.dtype == torch.uint8]
    assert len(saved) == 2 and len(packed) == 1 and any(t is w or t.data_ptr() == w.data_ptr() for t in saved)
    assert packed[0].numel() * packed[0].element_size() == cabi_x.quant_bytes(x.numel(), bits)
    assert torch.equal(packed[0].cpu(), cabi_x.quant_pack_host(x.detach().float().cpu(), seeds[0], bits))
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), gy)
    assert torch.equal(gx, gxr) and torch.equal(gb, gbr)
    assert gw.dtype == w.dtype and torch.equal(gw, weight_gradient_by(gy, x, seeds[0], bits, dtype).to(w.dtype))
    # and against the fp64 product of the fp32 decode, within the roundings of the dtype: of X^ (not at bf16 / 8 bits) and of the result
    decoded = decoded_by(x, seeds[0], bits, torch.float32).double()
    eps = 2.0**-8 if dtype == torch.bfloat16 else (shape[0] + 2) * 2.0**-24    # (fp32: the bound of a sum of `rows` products in fp32)
    assert bool(((gw.double() - gy.double().T @ decoded).abs() <= eps * (gy.double().abs().T @ decoded.abs())).all())
    # unbiased: over 200 seeds within 5 standard errors of the exact weight gradient, entry by entry
    exact = gy.double().T @ x.detach().double()
    calls = 200
    total, squares = torch.zeros_like(exact), torch.zeros_like(exact)
    layer = fewbit.QuantizedLinear(shape[1], shape[2], bits=bits, device=DEV, dtype=dtype)
    with torch.no_grad():
        layer.weight.copy_(w)
        layer.bias.copy_(b)
    for _ in range(calls):
        (g, ) = torch.autograd.grad(layer(x), layer.weight, gy)
        total += g.double()
        squares += g.double()**2
    assert len(seeds) == 1 + calls and len(set(seeds)) == len(seeds)
    mean = total / calls
    sd = (squares / calls - mean**2).clamp_min(0).sqrt() * math.sqrt(calls / (calls - 1))
    z = (mean - exact).abs() / (sd / math.sqrt(calls))
    print(f'{shape} {dtype} bits {bits}: worst entry {float(z.max()):.2f} standard errors; relative error of one call '
          f'{float((g.double() - exact).norm() / exact.norm()):.4f}')
    assert bool((sd > 0).all()) and float(z.max()) <= 5.0


@pytest.mark.parametrize('bits', BITS)
def test_three_dimensional_input_and_the_module(bits, seeds):
    layer = fewbit.QuantizedLinear(72, 40, bits=bits, device=DEV, dtype=torch.bfloat16)
    x = torch.randn(8, 25, 72, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    gy = torch.randn(8, 25, 40, device=DEV, dtype=torch.bfloat16)
    y = layer(x)
    gx, gw, gb = torch.autograd.grad(y, (x, layer.weight, layer.bias), gy)
    yr = F.linear(x, layer.weight, layer.bias)
    gxr, gbr = torch.autograd.grad(yr, (x, layer.bias), gy)
    assert torch.equal(y, yr) and torch.equal(gx, gxr) and torch.equal(gb, gbr)
    assert torch.equal(gw, weight_gradient_by(gy, x, seeds[0], bits, torch.bfloat16).to(torch.bfloat16))
    assert 'bits=%d' % bits in repr(layer)


def test_backward_may_follow_the_autocast_block(seeds):
    x, w, b, gy = problem(SHAPES[1], torch.float32, 1)
    with torch.autocast('cuda', dtype=torch.bfloat16):                # (a block of its own: autocast caches the cast of a weight per block)
        yr = F.linear(x, w, b)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        y = fewbit.functional.linear_quantized(x, w, b, 4)
    assert y.dtype == torch.bfloat16 and torch.equal(y, yr)
    g16 = gy.bfloat16()
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), g16)                # outside the block: the ordinary AMP pattern
    gxr, _, gbr = torch.autograd.grad(yr, (x, w, b), g16)
    assert gx.dtype == gw.dtype == gb.dtype == torch.float32
    assert torch.equal(gx, gxr)
    # (autocast runs `sum` in fp32: the bias gradient is the fp32 sum of the bf16 gradient, which F.linear's backward rounds to bf16 once more)
    assert torch.equal(gb, g16.float().sum(dim=0)) and bool(((gb - gbr).abs() <= 2.0**-8 * gb.abs()).all())
    # the fp32 input was packed as it is; X^ is decoded into the gradient's dtype
    assert torch.equal(gw, (g16.T @ decoded_by(x, seeds[0], 4, torch.bfloat16)).float())


@pytest.mark.parametrize('reentrant', (False, True))
def test_checkpointing_gives_the_plain_runs_bits(reentrant):
    x, w, b, gy = problem(SHAPES[1], torch.bfloat16, 2)
    torch.manual_seed(12)
    plain = torch.autograd.grad(fewbit.functional.linear_quantized(x, w, b, 4), (x, w, b), gy)
    torch.manual_seed(12)
    y = checkpoint(lambda t, weight, bias: fewbit.functional.linear_quantized(t, weight, bias, 4), x, w, b, use_reentrant=reentrant)
    x.grad = w.grad = b.grad = None
    y.backward(gy)
    for got, want in zip((x.grad, w.grad, b.grad), plain):
        assert torch.equal(got, want)
    x.grad = w.grad = b.grad = None


def test_layouts_no_grad_the_frozen_weight_and_the_switch(seeds):
    rows, fin, fout = SHAPES[1]
    _, w, b, gy = problem(SHAPES[1], torch.bfloat16, 3)
    base = torch.randn(fin, rows, device=DEV, dtype=torch.bfloat16)
    xt = base.t().requires_grad_()                                    # a non-contiguous input: packed from a contiguous copy
    y = fewbit.functional.linear_quantized(xt, w, b, 4)
    (gw, ) = torch.autograd.grad(y, w, gy)
    assert torch.equal(gw, gy.T @ decoded_by(base.t(), seeds[-1], 4, torch.bfloat16))
    # an expanded gradient (strides 0, 0) gives the result of its contiguous copy
    torch.manual_seed(5)
    (a, ) = torch.autograd.grad(fewbit.functional.linear_quantized(xt, w, b, 4).sum(), w)
    torch.manual_seed(5)
    (c, ) = torch.autograd.grad(fewbit.functional.linear_quantized(xt, w, b, 4), w, torch.ones(rows, fout, device=DEV, dtype=torch.bfloat16))
    assert torch.equal(a, c)
    # no_grad and a frozen weight: F.linear and nothing else
    count = len(seeds)
    with torch.no_grad():
        y, saved = saved_by(lambda: fewbit.functional.linear_quantized(xt, w, b, 4))
    assert y.grad_fn is None and not saved
    y, saved = saved_by(lambda: fewbit.functional.linear_quantized(xt, w.detach(), b, 4))
    assert 'Quantized' not in type(y.grad_fn).__name__ and not any(t.dtype == torch.uint8 for t in saved) and len(seeds) == count
    # the switch and float64: the PyTorch formulation, one code per byte
    prev = linear.use_native_sketch(False)
    try:
        y, saved = saved_by(lambda: fewbit.functional.linear_quantized(xt, w, b, 4))
    finally:
        linear.use_native_sketch(prev)
    assert len(seeds) == count and sorted(t.numel() for t in saved if t.dtype == torch.uint8) == [math.ceil(rows * fin / 64) * 64]
    (gw, ) = torch.autograd.grad(y, w, gy)
    exact = gy.double().T @ base.t().double()
    assert float((gw.double() - exact).norm() / exact.norm()) < 0.5
    xd = base.t().double().requires_grad_()
    y, saved = saved_by(lambda: fewbit.functional.linear_quantized(xd, w.double().detach().requires_grad_(), None, 8))
    assert len(seeds) == count and any(t.dtype == torch.uint8 for t in saved) and not any(t.shape == xd.shape for t in saved)


def test_a_captured_step_rounds_afresh_on_every_replay(monkeypatch):
    bits = 4
    x, w, b, gy = problem(SHAPES[0], torch.bfloat16, 4)

    def step():
        y = fewbit.functional.linear_quantized(x, w, b, bits)
        return torch.autograd.grad(y, (x, w), gy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                        # the eager warm-up: the per-device replay counter exists from here on
    torch.cuda.current_stream().wait_stream(side)
    bases = []
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: bases.append(0x1357924) or bases[-1])
    counter = linear._replay_counter(torch.device(DEV))
    torch.cuda.synchronize()
    c0 = int(counter)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gx, gw = step()
    assert len(bases) == 1 and int(counter) == c0
    gxr = gy @ w.detach()
    seen = []
    for replay in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert int(counter) == c0 + replay + 1
        assert torch.equal(gx, gxr)
        want = gy.T @ decoded_by(x, cabi.mix_sketch_seed(bases[0], c0 + replay), bits, torch.bfloat16)
        assert torch.equal(gw, want)                                  # the rounding of the seed the replay counter gave
        seen.append(gw.clone())
    assert not torch.equal(seen[0], seen[1])
