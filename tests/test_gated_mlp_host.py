"""The gated MLP as one node without a GPU (fewbit_amd/glu.py, ``gated_mlp_quantized``; include/fewbit_hipx.h, ``fewbit_hipx_glu_backward_product``):
the new entry point (declared, exported, bound, refusing), the expectation of the rebuilt product ``act(g^) u^`` over many seeds and the independence
of the roundings of ``x`` and of ``gate`` under their two seeds, the node on host tensors (what it computes, what it keeps, what it keeps when only
some gradients are asked for), and ``QuantizedGatedMLP(fused=...)`` inside ``from_mlp``, ``map_module`` and both checkpoint modes."""
import math
import re
import subprocess
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

import fewbit
from fewbit_amd import cabi, cabi_x
from gated_mlp_harness import StubBlock, StubMLP, exact_mlp, levels_of, parameters_of, tame
from glu_harness import act64, decoded, halves
from norm_harness import saved_by, seeds  # noqa: F401  (a fixture)

ROOT = Path(__file__).resolve().parents[1]
BITS = (2, 4, 8)
SILU = cabi.CONTINUOUS.index('silu')
P = 0x10000                                                         # a 16-byte aligned address that is never dereferenced


# ---- the entry point ------------------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_exported_declared_and_bound_and_the_revision_is_still_2():
    name = 'fewbit_hipx_glu_backward_product'
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    declared = set(re.findall(r'\b(fewbit_hipx_\w+)\s*\(', header))
    out = subprocess.run(['nm', '-D', '--defined-only', str(cabi_x.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert name in declared and name in exported and name in cabi_x.SYMBOLS
    assert cabi_x.lib().fewbit_hipx_revision() == cabi_x.REVISION == 2 and cabi_x.lib().fewbit_hipx_abi_version() == cabi_x.ABI_VERSION == 1
    assert 'glu_backward_product' in cabi_x.__all__
    assert 'product[i] = round_to_dtype(act(g^) * u^)' in header and 'gy may be NULL only' in header
    assert fewbit.functional.gated_mlp_quantized is fewbit.glu.gated_mlp_quantized is fewbit.gated_mlp_quantized


def refused(rc, *words):
    message = cabi_x.lib().fewbit_hipx_last_error().decode()
    assert rc == -1 and all(word in message for word in words), (rc, message)


def test_the_entry_point_refuses_before_it_launches():
    """(no device is touched: the pointers are never read)"""
    f = cabi_x.lib().fewbit_hipx_glu_backward_product
    ok = dict(dtype=1, act=SILU, gy=P, state=2 * P, rows=4, width=64, bits=8, d_gate=3 * P, ld_dgate=128, d_up=3 * P + 128, ld_dup=128, product=4 * P, ld_product=64,
              stream=None)

    def call(**changes):
        return f(*{**ok, **changes}.values())

    refused(call(dtype=-1), 'unknown dtype')
    refused(call(act=cabi.CONTINUOUS.index('celu')), 'neither FEWBIT_SILU nor FEWBIT_GELU')
    refused(call(bits=0), 'bits = 0')
    refused(call(bits=3), 'bits = 3')
    refused(call(width=0), 'outside 1 .. 2^36')
    refused(call(rows=2**20, width=2**20), 'outside 1 .. 2^36')
    refused(call(ld_dgate=63), 'below the width')
    refused(call(ld_dup=0), 'below the width')
    refused(call(ld_product=63), 'below the width')
    refused(call(state=None), 'null')
    refused(call(gy=None), 'gy is a null pointer and a gradient is wanted')
    refused(call(gy=None, d_gate=None), 'gy is a null pointer and a gradient is wanted')
    refused(call(gy=None, d_up=None), 'gy is a null pointer and a gradient is wanted')
    for name in ('gy', 'd_gate', 'd_up', 'product'):
        refused(call(**{name: P + 1}), 'aligned to their element')
    refused(call(state=2 * P + 4), 'state must be 8-byte aligned')
    assert call(rows=0) == 0
    assert call(d_gate=None, d_up=None, product=None) == 0          # nothing is wanted: nothing is launched
    assert call(gy=None, d_gate=None, ld_dgate=0, d_up=None, ld_dup=0, product=None, ld_product=0) == 0


def test_the_binding_refuses_host_tensors_unknown_activations_and_other_bits():
    x, state = torch.zeros(4, 8), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(cabi_x.FewbitHipError, match='must live on the GPU'):
        cabi_x.glu_backward_product(x, state, 'silu', 4)
    with pytest.raises(cabi_x.FewbitHipError, match='must live on the GPU'):
        cabi_x.glu_backward_product(None, state, 'silu', 4, (False, False, True), product=x)
    with pytest.raises(cabi_x.FewbitHipError, match="'silu' or 'gelu'"):
        cabi_x.glu_backward_product(x, state, 'gelu_tanh', 4)
    for bits in (0, 3, 16):
        with pytest.raises(cabi_x.FewbitHipError, match='bits must be 2, 4 or 8'):
            cabi_x.glu_backward_product(x, state, 'silu', bits)
    with pytest.raises(cabi_x.FewbitHipError, match='neither d_gate nor d_up'):
        cabi_x.glu_backward_product(None, state, 'silu', 4, (True, False, True), product=x)
    with pytest.raises(cabi_x.FewbitHipError, match='product buffer must be given'):
        cabi_x.glu_backward_product(None, state, 'silu', 4, (False, False, True))
    assert cabi_x.glu_backward_product(None, state, 'silu', 4, (False, False, False)) == (None, None, None)


# ---- the expectation of the rebuilt product, the independence of the two seeds ---------------------------------------------------------------------
CALLS = 1000
GOLDEN = 0x9E3779B97F4A7C15


@pytest.mark.parametrize('activation', ('silu', 'gelu'))
@pytest.mark.parametrize('bits', BITS)
def test_the_mean_product_of_many_seeds_is_the_stated_expectation(bits, activation):
    """E[y^] = ((1 - f_g) act(g0) + f_g act(g1)) ((1 - f_u) u0 + f_u u1), the two roundings of one seed being independent: the mean over CALLS seeds of
    act64(g^) u^ on the host evaluation lies within 5 standard errors at every element (an element without variance: to rounding).  The setup is
    that of tests/test_glu_host.py: tamed inputs, whose variances are at least 0.1275 step^2 where they are not 0."""
    n = 256
    g = torch.Generator().manual_seed(5 + bits)
    gate, up = tame(1.5 * torch.randn(n, generator=g), bits, g), tame(1.5 * torch.randn(n, generator=g), bits, g)
    first, second, _ = halves(cabi_x.glu_state_host(gate, up, 0, bits), n, bits)
    par_g, par_u = first[:8 * (n // 64)].view(torch.float32).numpy(), second[:8 * (n // 64)].view(torch.float32).numpy()
    g0, g1, fg = (torch.from_numpy(a) for a in levels_of(gate.numpy(), par_g[0::2], par_g[1::2], bits))
    u0, u1, fu = (torch.from_numpy(a) for a in levels_of(up.numpy(), par_u[0::2], par_u[1::2], bits))
    want = ((1 - fg) * act64(g0, activation) + fg * act64(g1, activation)) * ((1 - fu) * u0 + fu * u1)
    samples = []
    for seed in range(CALLS):
        gq, uq = decoded(cabi_x.glu_state_host(gate, up, seed * GOLDEN + 1, bits), n, bits)
        samples.append(act64(gq, activation) * uq.double())
    samples = torch.stack(samples)
    mean, sd = samples.mean(dim=0), samples.std(dim=0)
    still = sd == 0
    assert int(still.sum()) <= 2 * (n // 64) + 2                                             # (elements where both factors are extremes of their groups)
    assert bool(((mean - want).abs()[still] <= 1e-6 * want.abs()[still] + 1e-12).all())
    z = ((mean - want).abs() / (sd / math.sqrt(CALLS)))[~still]
    print(f'{activation} bits {bits} product: worst element {float(z.max()):.2f} standard errors')
    assert float(z.max()) <= 5.0


@pytest.mark.parametrize('bits', BITS)
def test_the_roundings_of_x_and_of_gate_under_two_seeds_are_uncorrelated(bits):
    """x^ - x (the packed form of seed_x) against g^ - g (the gate part of the state of seed_gu) at equal flat indices, over CALLS pairs of seeds: the
    sample correlation of every element lies within 5 / sqrt(CALLS) of 0.  Both round in counter domain 7, so the sharpest case is x = gate: with ONE
    seed the two errors are the same numbers (correlation 1, shown on a few seeds), which is why the node draws two."""
    n = 256
    g = torch.Generator().manual_seed(40 + bits)
    values = tame(1.5 * torch.randn(n, generator=g), bits, g)
    up = torch.randn(n, generator=g)
    ex, eg = [], []
    for call in range(CALLS):
        seed_x, seed_gu = (2 * call) * GOLDEN + 1, (2 * call + 1) * GOLDEN + 1
        ex.append(cabi_x.quant_unpack_host(cabi_x.quant_pack_host(values, seed_x, bits), n, bits).double() - values.double())
        eg.append(decoded(cabi_x.glu_state_host(values, up, seed_gu, bits), n, bits)[0].double() - values.double())
    ex, eg = torch.stack(ex), torch.stack(eg)
    moving = (ex.std(dim=0) > 0) & (eg.std(dim=0) > 0)
    assert int((~moving).sum()) <= 2 * (n // 64) + 2
    cx, cg = ex - ex.mean(dim=0), eg - eg.mean(dim=0)
    correlation = ((cx * cg).sum(dim=0) / (cx.norm(dim=0) * cg.norm(dim=0)).clamp_min(1e-300))[moving]
    print(f'bits {bits}: largest correlation {float(correlation.abs().max()):.4f} (allowed {5 / math.sqrt(CALLS):.4f})')
    assert float(correlation.abs().max()) <= 5 / math.sqrt(CALLS)
    for seed in (1, 2, 3):
        same = cabi_x.quant_unpack_host(cabi_x.quant_pack_host(values, seed, bits), n, bits)
        assert torch.equal(same, decoded(cabi_x.glu_state_host(values, up, seed, bits), n, bits)[0])


# ---- the node on host tensors ------------------------------------------------------------------------------------------------------------------------
SHAPES = (((2, 12, 40), 72), ((5, 24), 100))


def problem(shape, hidden, dtype, bias=True, salt=0):
    torch.manual_seed(17 + salt)
    mlp = fewbit.QuantizedGatedMLP(shape[-1], hidden, bias=bias, bits=8, dtype=dtype, fused=True)
    g = torch.Generator().manual_seed(29 + salt)
    return mlp, torch.randn(*shape, generator=g).to(dtype).requires_grad_(), torch.randn(*shape, generator=g).to(dtype)


def call_of(mlp, x, activation='silu', bits=8):
    p = mlp
    return fewbit.functional.gated_mlp_quantized(x, p.gate_proj.weight, p.up_proj.weight, p.down_proj.weight, p.gate_proj.bias, p.up_proj.bias, p.down_proj.bias,
                                                 activation, bits)


def kept_only_codes_parameters_and_weights(saved, mlp, rows, width, hidden, with_x=True):
    """the saved tensors: uint8 codes, fp32 / fp64 parameters of groups of 64, the three weights -- nothing of T x I or T x H in a float dtype"""
    weights = [p for name, p in parameters_of(mlp) if name.endswith('weight')]
    others = [t for t in saved if not any(t is w for w in weights)]
    assert sum(any(t is w for w in weights) for t in saved) == 3
    pad = lambda n: math.ceil(n / 64) * 64
    codes = sorted(t.numel() for t in others if t.dtype == torch.uint8)
    assert codes == sorted(([pad(rows * width)] if with_x else []) + 2 * [pad(rows * hidden)])
    floats = [t for t in others if t.dtype != torch.uint8]
    assert sorted(t.numel() for t in floats) == sorted((2 * [pad(rows * width) // 64] if with_x else []) + 4 * [pad(rows * hidden) // 64])
    assert not any(t.is_floating_point() and t.numel() >= min(rows * width, rows * hidden) for t in others)


@pytest.mark.parametrize('activation', ('silu', 'gelu'))
@pytest.mark.parametrize('dtype', (torch.float32, torch.float64))
@pytest.mark.parametrize('shape,hidden', SHAPES)
def test_the_host_path_gives_the_exact_output_keeps_codes_alone_and_close_gradients(shape, hidden, dtype, activation):
    """The output is torch's composition to the bit.  At 8 bits an element of x^, g^ or u^ is moved by at most a step, 1 / 255 of its group's range:
    tests/test_glu_host.py allows the product's own gradients 0.05 and 0.1 of their scale for that; every gradient here is a sum over the tokens of
    products of such terms with independent errors of mean 0, so the larger allowance, 0.1 of the gradient's largest element, holds each of them."""
    mlp, x, gy = problem(shape, hidden, dtype)
    torch.manual_seed(3)
    out, saved = saved_by(lambda: call_of(mlp, x, activation))
    exact = exact_mlp(x, mlp, activation)
    assert torch.equal(out, exact.detach()) and type(out.grad_fn).__name__ == '_GatedMLPQuantizedBackward' and out.shape == x.shape
    rows = x.numel() // shape[-1]
    kept_only_codes_parameters_and_weights(saved, mlp, rows, shape[-1], hidden)
    names, parameters = zip(*([('x', x)] + parameters_of(mlp)))
    got = torch.autograd.grad(out, parameters, gy)
    want = torch.autograd.grad(exact, parameters, gy)
    for name, a, b in zip(names, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and bool(torch.isfinite(a).all()), name
        error = float((a - b).abs().max()) / float(b.abs().max())
        print(f'{name}: error {error:.4f} of the largest element')
        assert error <= 0.1, name
    # the bias gradient of down_proj is exact
    assert torch.equal(got[-1], want[-1])
    with pytest.raises(RuntimeError):                               # once_differentiable: no second derivative
        gg, = torch.autograd.grad(call_of(mlp, x, activation), x, gy, create_graph=True)
        gg.sum().backward()


def test_the_refusals_of_the_function():
    mlp, x, _ = problem((5, 24), 100, torch.float32)
    with pytest.raises(ValueError, match='bits should be 2, 4 or 8'):
        call_of(mlp, x, bits=3)
    with pytest.raises(ValueError, match="'silu' or 'gelu'"):
        call_of(mlp, x, activation='relu')


# ---- what is kept when only some gradients are asked for, and the modes -----------------------------------------------------------------------------
def test_nothing_is_kept_that_no_requested_gradient_needs(seeds):  # noqa: F811
    shape, hidden = (2, 12, 40), 72
    mlp, x, gy = problem(shape, hidden, torch.float32)
    rows = 24
    exact = exact_mlp(x, mlp, 'silu').detach()
    out, saved = saved_by(lambda: mlp(x))
    assert torch.equal(out, exact) and len(saved) == 12 and len(seeds) == 0         # (the host formulation draws from the generator, not a seed)
    # grad mode off, and nothing that requires grad: the plain forward, nothing kept, nothing drawn
    state = torch.get_rng_state()
    with torch.no_grad():
        out, saved = saved_by(lambda: mlp(x))
    assert out.grad_fn is None and not saved and torch.equal(out, exact) and torch.equal(torch.get_rng_state(), state)
    mlp.requires_grad_(False)
    out, saved = saved_by(lambda: mlp(x.detach()))
    assert out.grad_fn is None and not saved and torch.equal(out, exact) and torch.equal(torch.get_rng_state(), state)
    # x alone: no gradient needs x^
    out, saved = saved_by(lambda: mlp(x))
    assert torch.equal(out, exact)
    kept_only_codes_parameters_and_weights(saved, mlp, rows, 40, hidden, with_x=False)
    dx, = torch.autograd.grad(out, x, gy)
    want, = torch.autograd.grad(exact_mlp(x, mlp, 'silu'), x, gy)
    assert float((dx - want).abs().max()) <= 0.1 * float(want.abs().max())
    # the weight of down_proj alone: the state of gate and up (for y^), no x^
    mlp.down_proj.weight.requires_grad_(True)
    out, saved = saved_by(lambda: mlp(x.detach()))
    assert torch.equal(out, exact)
    kept_only_codes_parameters_and_weights(saved, mlp, rows, 40, hidden, with_x=False)
    got, = torch.autograd.grad(out, mlp.down_proj.weight, gy)
    want, = torch.autograd.grad(exact_mlp(x.detach(), mlp, 'silu'), mlp.down_proj.weight, gy)
    assert float((got - want).abs().max()) <= 0.1 * float(want.abs().max())
    # the bias of down_proj alone: its gradient is a column sum of the incoming gradient, no state at all
    mlp.requires_grad_(False)
    mlp.down_proj.bias.requires_grad_(True)
    out, saved = saved_by(lambda: mlp(x.detach()))
    assert torch.equal(out, exact) and len(saved) == 3
    assert torch.equal(torch.autograd.grad(out, mlp.down_proj.bias, gy)[0], gy.reshape(-1, 40).sum(dim=0))
    # the weight of gate_proj alone: x^ and the state
    mlp.requires_grad_(False)
    mlp.gate_proj.weight.requires_grad_(True)
    out, saved = saved_by(lambda: mlp(x.detach()))
    kept_only_codes_parameters_and_weights(saved, mlp, rows, 40, hidden, with_x=True)
    # eval: torch's exact product and its exact gradients, nothing rounded or drawn
    mlp.requires_grad_(True)
    mlp.eval()
    state = torch.get_rng_state()
    out, saved = saved_by(lambda: mlp(x))
    assert 'GatedMLPQuantized' not in type(out.grad_fn).__name__ and not any(t.dtype == torch.uint8 for t in saved) and torch.equal(torch.get_rng_state(), state)
    parameters = [x] + [p for _, p in parameters_of(mlp)]
    assert all(torch.equal(a, b) for a, b in zip(torch.autograd.grad(out, parameters, gy), torch.autograd.grad(exact_mlp(x, mlp, 'silu'), parameters, gy)))
    with torch.no_grad():
        assert torch.equal(mlp(x), exact)
    assert 'fused=True' in repr(mlp) and 'fused=False' in repr(fewbit.QuantizedGatedMLP(4, 8))


def test_the_default_saves_what_it_saved_before():
    """``fused=False``: three ``nn.Linear`` layers around the product node -- x twice, the six tensors of the product's codes, y, and the weights"""
    torch.manual_seed(0)
    mlp = fewbit.QuantizedGatedMLP(16, 40, bits=4)
    assert mlp.fused is False
    x = torch.randn(6, 16, requires_grad=True)
    out, saved = saved_by(lambda: mlp(x))
    # (torch's linear saves the transposed view of its weight: 16 x 40 for gate_proj and up_proj, 40 x 16 for down_proj)
    assert sorted(tuple(t.shape) for t in saved) == sorted([(6, 16), (16, 40), (6, 16), (16, 40), (256, ), (4, ), (4, ), (256, ), (4, ), (4, ), (6, 40), (40, 16)])
    assert [t.dtype for t in saved].count(torch.uint8) == 2
    torch.manual_seed(0)
    fused = fewbit.QuantizedGatedMLP(16, 40, bits=4, fused=True)
    out2, saved = saved_by(lambda: fused(x))
    assert torch.equal(out, out2)
    assert sorted(tuple(t.shape) for t in saved) == sorted([(128, ), (2, ), (2, ), (40, 16), (40, 16), (256, ), (4, ), (4, ), (256, ), (4, ), (4, ), (16, 40)])


@pytest.mark.parametrize('act_fn,name', ((torch.nn.SiLU(), 'silu'), (F.gelu, 'gelu')))
def test_from_mlp_shares_the_projections_of_a_stub_with_the_flag(act_fn, name):
    torch.manual_seed(0)
    stub = StubMLP(act_fn)
    mlp = fewbit.QuantizedGatedMLP.from_mlp(stub, bits=8, fused=True)
    assert mlp.fused and mlp.glu.activation == name and mlp.glu.bits == 8 and mlp.training
    assert mlp.gate_proj.weight is stub.gate_proj.weight and mlp.up_proj.weight is stub.up_proj.weight and mlp.down_proj.weight is stub.down_proj.weight
    assert len(list(mlp.parameters())) == 3 and not any(p.is_meta for p in mlp.parameters())
    assert not fewbit.QuantizedGatedMLP.from_mlp(stub).fused
    x = torch.randn(6, 16, requires_grad=True)
    y, saved = saved_by(lambda: mlp(x))
    assert torch.equal(y, stub(x)) and type(y.grad_fn).__name__ == '_GatedMLPQuantizedBackward' and sum(t.dtype == torch.uint8 for t in saved) == 3
    for p in stub.parameters():
        got = torch.autograd.grad(mlp(x).sum(), p)[0]
        want = torch.autograd.grad(stub(x).sum(), p)[0]
        assert float((got - want).abs().max()) <= 0.05 * float(want.abs().max()) + 1e-3


def test_map_module_swaps_the_mlp_of_a_llama_style_model():
    torch.manual_seed(1)
    model = torch.nn.Sequential(StubBlock(), StubBlock())
    x = torch.randn(7, 16)
    want = model(x)
    swap = lambda m, path: fewbit.QuantizedGatedMLP.from_mlp(m, bits=4, fused=True) if type(m).__name__.endswith('MLP') else m
    model = fewbit.map_module(model, swap)
    assert all(type(block.mlp) is fewbit.QuantizedGatedMLP and block.mlp.fused for block in model)
    y, saved = saved_by(lambda: model(x))
    assert torch.equal(y, want) and sum(t.dtype == torch.uint8 for t in saved) == 6
    y.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


@pytest.mark.parametrize('reentrant', (False, True))
def test_checkpointing_gives_the_plain_runs_bits(reentrant):
    mlp, x, gy = problem((2, 12, 40), 72, torch.float32, salt=2)
    parameters = [p for _, p in parameters_of(mlp)]
    torch.manual_seed(12)
    out0 = mlp(x)
    plain = torch.autograd.grad(out0, [x] + parameters, gy)
    torch.manual_seed(12)
    out = checkpoint(mlp, x, use_reentrant=reentrant)
    out.backward(gy)
    assert torch.equal(out, out0) and torch.equal(x.grad, plain[0])
    assert all(torch.equal(p.grad, g) for p, g in zip(parameters, plain[1:]))
