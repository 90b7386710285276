"""The gate and the up of a seed without a GPU (include/fewbit_hipx.h; fewbit_amd/csrc/fewbit_glu.hip): the four entry points of the companion
library (declared, exported, bound), the host evaluation against ``quant_pack_host`` (the gate part) and against a numpy restatement with
rounding domain 8 (the up part), the size formula and the zero bytes, the refusals before anything is launched, the expectation of both
gradients over many seeds, poisoned and constant groups, and ``fewbit.QuantizedGLU`` / ``QuantizedGatedMLP`` on host tensors."""
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

import fewbit
from fewbit_amd import cabi, cabi_x
from glu_harness import GATE_DOMAIN, UP_DOMAIN, act64, decoded, halves, part_bytes, restated, slope64, uniforms
from norm_harness import saved_by, seeds  # noqa: F401  (a fixture)

ROOT = Path(__file__).resolve().parents[1]
GLU_SYMBOLS = ('fewbit_hipx_glu_state_bytes', 'fewbit_hipx_glu_state_host', 'fewbit_hipx_glu_forward', 'fewbit_hipx_glu_backward')
BITS = (2, 4, 8)
SIZES = (1, 7, 8, 9, 63, 64, 65, 205, 2573)
SEED = 0x1234567887654321
SILU, GELU, CELU = cabi.CONTINUOUS.index('silu'), cabi.CONTINUOUS.index('gelu'), cabi.CONTINUOUS.index('celu')


def draw(n, salt=0, scale=3.0):
    g = torch.Generator().manual_seed(91 + salt)
    return scale * torch.randn(n, generator=g), scale * torch.randn(n, generator=g)


# ---- the library: symbols, sizes, the definition ------------------------------------------------------------------------------------------------
def test_the_four_symbols_are_exported_declared_and_bound_and_the_revision_is_still_2():
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    declared = set(re.findall(r'\b(fewbit_hipx_\w+)\s*\(', header))
    out = subprocess.run(['nm', '-D', '--defined-only', str(cabi_x.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in GLU_SYMBOLS:
        assert name in declared and name in exported and name in cabi_x.SYMBOLS, name
    assert declared == set(cabi_x.SYMBOLS) == {name for name in exported if name.startswith('fewbit_hipx_')}
    assert cabi_x.lib().fewbit_hipx_revision() == cabi_x.REVISION == 2 and cabi_x.lib().fewbit_hipx_abi_version() == cabi_x.ABI_VERSION == 1
    assert 'The gate and the up of a seed' in header and 'second order in the step (d_up through act, d_gate through act\')' in header
    assert {'glu_state_bytes', 'glu_state_host', 'glu_forward', 'glu_backward'} <= set(cabi_x.__all__)
    assert fewbit.functional.glu_quantized is fewbit.glu.glu_quantized and fewbit.QuantizedGLU and fewbit.QuantizedGatedMLP


def test_state_bytes_is_two_parts_of_the_packed_form_filled_up_to_eight():
    for bits in BITS:
        for n in SIZES + (2**22, 2**36):
            part = 8 * math.ceil((8 * math.ceil(n / 64) + bits * math.ceil(n / 8)) / 8)
            assert cabi_x.glu_state_bytes(n, bits) == 2 * part == 2 * part_bytes(n, bits), (n, bits)
            assert 0 <= part - cabi_x.quant_bytes(n, bits) < 8
        assert cabi_x.glu_state_bytes(0, bits) == 0 and cabi_x.glu_state_bytes(2**36 + 1, bits) == 0 and cabi_x.glu_state_bytes(-1, bits) == 0
    for bits in (0, 1, 3, 5, 16):
        assert cabi_x.glu_state_bytes(64, bits) == 0, bits
    # relative to two bf16 inputs: the table of the documents
    n = 2**20
    assert [cabi_x.glu_state_bytes(n, b) / (4 * n) for b in BITS] == [0.1875, 0.3125, 0.5625]


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('bits', BITS)
def test_the_gate_part_is_quant_pack_host_and_the_up_part_the_same_definition_in_domain_8(bits, n):
    gate, up = draw(n, n)
    for seed in (SEED, 7):
        state = cabi_x.glu_state_host(gate, up, seed, bits)
        first, second, padding = halves(state, n, bits)
        assert torch.equal(first, cabi_x.quant_pack_host(gate, seed, bits))
        assert np.array_equal(first.numpy(), restated(gate.numpy(), bits, seed, GATE_DOMAIN))
        want = restated(up.numpy(), bits, seed, UP_DOMAIN)
        assert np.array_equal(second.numpy(), want), (seed, np.flatnonzero(second.numpy() != want)[:8])
        assert not padding.any()
    # one tensor in both places: the same parameters, other roundings
    state = cabi_x.glu_state_host(gate, gate, SEED, bits)
    first, second, _ = halves(state, n, bits)
    groups = math.ceil(n / 64)
    assert torch.equal(first[:8 * groups], second[:8 * groups])
    assert n < 8 or not torch.equal(first, second)
    assert not np.array_equal(uniforms(64, SEED, GATE_DOMAIN), uniforms(64, SEED, UP_DOMAIN))


def test_the_host_function_does_not_write_behind_the_state():
    for bits in BITS:
        gate, up = draw(65)
        need = cabi_x.glu_state_bytes(65, bits)
        buffer = torch.full((need + 64, ), 0xA5, dtype=torch.uint8)
        g, u = gate.contiguous(), up.contiguous()
        assert cabi_x.lib().fewbit_hipx_glu_state_host(g.data_ptr(), u.data_ptr(), 65, bits, SEED, buffer.data_ptr()) == 0
        assert torch.equal(buffer[:need], cabi_x.glu_state_host(gate, up, SEED, bits)) and bool((buffer[need:] == 0xA5).all())


# ---- the refusals, before anything is launched (no device is touched: the pointers are never read) ---------------------------------------------------
P = 0x10000                                                         # a 16-byte aligned address that is never dereferenced


def refused(rc, *words):
    message = cabi_x.lib().fewbit_hipx_last_error().decode()
    assert rc == -1 and all(word in message for word in words), (rc, message)


def test_the_host_function_refuses():
    L = cabi_x.lib()
    x = torch.zeros(64)
    out = torch.zeros(256, dtype=torch.uint8)
    refused(L.fewbit_hipx_glu_state_host(x.data_ptr(), x.data_ptr(), 64, 3, 0, out.data_ptr()), 'bits = 3')
    refused(L.fewbit_hipx_glu_state_host(x.data_ptr(), x.data_ptr(), 2**36 + 1, 4, 0, out.data_ptr()), '2^36')
    refused(L.fewbit_hipx_glu_state_host(None, x.data_ptr(), 64, 4, 0, out.data_ptr()), 'null')
    refused(L.fewbit_hipx_glu_state_host(x.data_ptr(), None, 64, 4, 0, out.data_ptr()), 'null')
    refused(L.fewbit_hipx_glu_state_host(x.data_ptr(), x.data_ptr(), 64, 4, 0, None), 'null')
    assert L.fewbit_hipx_glu_state_host(None, None, 0, 4, 0, None) == 0
    with pytest.raises(cabi_x.FewbitHipError, match='bits must be 2, 4 or 8'):
        cabi_x.glu_state_host(x, x, 0, 3)
    with pytest.raises(cabi_x.FewbitHipError, match='one shape'):
        cabi_x.glu_state_host(x, x[:63], 0, 4)


def test_forward_refuses_before_it_launches():
    f = cabi_x.lib().fewbit_hipx_glu_forward
    ok = dict(dtype=2, act=SILU, gate=P, ld_gate=64, up=2 * P, ld_up=64, rows=4, width=64, bits=4, seed=0, seed_device=None, y=3 * P, state=4 * P,
              state_bytes=cabi_x.glu_state_bytes(256, 4), stream=None)

    def call(**changes):
        return f(*{**ok, **changes}.values())

    refused(call(dtype=3), 'unknown dtype')
    refused(call(act=CELU), 'neither FEWBIT_SILU nor FEWBIT_GELU')
    refused(call(act=99), 'neither FEWBIT_SILU nor FEWBIT_GELU')
    refused(call(bits=3), 'bits = 3')
    refused(call(seed_device=P + 4), 'seed word')
    refused(call(width=0), 'outside 1 .. 2^36')
    refused(call(rows=2**30, width=2**30), 'outside 1 .. 2^36')
    refused(call(rows=2**63, width=4), 'outside 1 .. 2^36')
    refused(call(ld_gate=63), 'below the width')
    refused(call(ld_up=8), 'below the width')
    for name in ('gate', 'up', 'y'):
        refused(call(**{name: None}), 'null')
        refused(call(**{name: P + 1}), 'aligned to their element')
    refused(call(state=4 * P + 4), 'state must be 8-byte aligned')
    refused(call(state_bytes=ok['state_bytes'] - 1), 'are needed')
    assert call(rows=0) == 0 and call(rows=0, gate=None, up=None, y=None, state=None) == 0
    # without a state bits and the seed word are not looked at, the rest is
    refused(call(state=None, bits=3, seed_device=P + 4, dtype=7), 'unknown dtype')
    refused(call(state=None, bits=3, seed_device=P + 4, ld_gate=1), 'below the width')


def test_backward_refuses_before_it_launches():
    f = cabi_x.lib().fewbit_hipx_glu_backward
    ok = dict(dtype=1, act=GELU, gy=P, state=2 * P, rows=4, width=64, bits=8, d_gate=3 * P, ld_dgate=128, d_up=3 * P + 128, ld_dup=128, stream=None)

    def call(**changes):
        return f(*{**ok, **changes}.values())

    refused(call(dtype=-1), 'unknown dtype')
    refused(call(act=CELU), 'neither FEWBIT_SILU nor FEWBIT_GELU')
    refused(call(bits=0), 'bits = 0')
    refused(call(width=0), 'outside 1 .. 2^36')
    refused(call(rows=2**20, width=2**20), 'outside 1 .. 2^36')
    refused(call(ld_dgate=63), 'below the width')
    refused(call(ld_dup=0), 'below the width')
    refused(call(gy=None), 'null')
    refused(call(state=None), 'null')
    for name in ('gy', 'd_gate', 'd_up'):
        refused(call(**{name: P + 1}), 'aligned to their element')
    refused(call(state=2 * P + 4), 'state must be 8-byte aligned')
    assert call(rows=0) == 0
    assert call(d_gate=None, d_up=None) == 0                        # nothing is wanted: nothing is launched
    assert call(d_gate=None, ld_dgate=0, d_up=None, ld_dup=0) == 0


def test_the_bindings_refuse_host_tensors_and_unknown_activations():
    x = torch.zeros(4, 8)
    with pytest.raises(cabi_x.FewbitHipError, match='must live on the GPU'):
        cabi_x.glu_forward(x, x)
    with pytest.raises(cabi_x.FewbitHipError, match='must live on the GPU'):
        cabi_x.glu_backward(x, torch.zeros(64, dtype=torch.uint8), 'silu', 4)


# ---- the expectation of both gradients --------------------------------------------------------------------------------------------------------------
CALLS = 1000


def levels_of(x, lo, step, bits):
    """(v0, v1, f) of every element, float64: the two neighbouring decodes and the probability of the upper one, from lo, step and the fp32 t of the
    definition"""
    L = np.float32(2**bits - 1)
    lo, step = np.repeat(lo, 64)[:x.size], np.repeat(step, 64)[:x.size]
    with np.errstate(all='ignore'):
        span = (step.astype(np.float64) * float(L))
        hi = np.array([x[i:i + 64].max() for i in range(0, x.size, 64)], dtype=np.float32)
        rng = (np.repeat(hi, 64)[:x.size] - lo).astype(np.float32)
        inv = np.where(rng > 0, (L / rng).astype(np.float32), np.float32(0))
    del span
    t = ((x - lo).astype(np.float32) * inv).astype(np.float32)
    k = np.minimum(np.floor(t), L - 1).astype(np.float64)          # (the maximum of a group: t = L exactly, code L with certainty -- f = 1 over level L - 1)
    f = t.astype(np.float64) - k
    fma = lambda code: (code * step.astype(np.float64) + lo.astype(np.float64)).astype(np.float32).astype(np.float64)
    return fma(k), fma(k + 1), f


def tame(x, bits, generator):
    """`x` with every element but its group's minimum and maximum moved to a level plus a fraction in [0.15, 0.85] of a step: every variance that is
    not exactly 0 is then at least 0.1275 step^2, far above the 2^-16 granularity of U"""
    x = x.clone().view(-1, 64)
    L = 2**bits - 1
    lo, hi = x.amin(dim=1, keepdim=True), x.amax(dim=1, keepdim=True)
    step = (hi - lo) / L
    k = torch.randint(0, L, x.shape, generator=generator)
    f = 0.15 + 0.7 * torch.rand(x.shape, generator=generator)
    moved = lo + (k + f) * step
    keep = (x == lo) | (x == hi)
    return torch.where(keep, x, moved).reshape(-1)


@pytest.mark.parametrize('activation', ('silu', 'gelu'))
@pytest.mark.parametrize('bits', BITS)
def test_the_mean_gradients_of_many_seeds_are_the_stated_expectations(bits, activation):
    """E[d_up] = gy ((1 - f) act(v0) + f act(v1)) and, the two roundings being independent, E[d_gate] = gy E[u^] ((1 - f) act'(v0) + f act'(v1)): the
    mean over CALLS seeds of the host evaluation lies within 5 standard errors at every element (an element without variance: to rounding).  The
    2^-16 granularity of U moves f by at most 2^-16 where a standard error is at least sqrt(0.1275 / 1000) = 0.011 of the same difference: a
    seven-hundredth of it."""
    n = 256
    g = torch.Generator().manual_seed(5 + bits)
    gate, up = tame(1.5 * torch.randn(n, generator=g), bits, g), tame(1.5 * torch.randn(n, generator=g), bits, g)
    gy = torch.randn(n, generator=g).double()
    state = cabi_x.glu_state_host(gate, up, 0, bits)
    first, second, _ = halves(state, n, bits)
    par_g, par_u = first[:8 * (n // 64)].view(torch.float32).numpy(), second[:8 * (n // 64)].view(torch.float32).numpy()
    g0, g1, fg = (torch.from_numpy(a) for a in levels_of(gate.numpy(), par_g[0::2], par_g[1::2], bits))
    u0, u1, fu = (torch.from_numpy(a) for a in levels_of(up.numpy(), par_u[0::2], par_u[1::2], bits))
    want_up = gy * ((1 - fg) * act64(g0, activation) + fg * act64(g1, activation))
    want_gate = gy * ((1 - fu) * u0 + fu * u1) * ((1 - fg) * slope64(g0, activation) + fg * slope64(g1, activation))
    d_up, d_gate = [], []
    for seed in range(CALLS):
        gq, uq = decoded(cabi_x.glu_state_host(gate, up, seed * 0x9E3779B97F4A7C15 + 1, bits), n, bits)
        assert bool(((gq.double() == g0) | (gq.double() == g1)).all()) and bool(((uq.double() == u0) | (uq.double() == u1)).all())
        d_up.append(gy * act64(gq, activation))
        d_gate.append(gy * uq.double() * slope64(gq, activation))
    worst = 0.0
    for name, samples, want in (('d_up', torch.stack(d_up), want_up), ('d_gate', torch.stack(d_gate), want_gate)):
        mean, sd = samples.mean(dim=0), samples.std(dim=0)
        still = sd == 0
        assert int(still.sum()) <= 2 * (n // 64) + 2, name                                   # (the extremes of the groups)
        assert bool(((mean - want).abs()[still] <= 1e-6 * want.abs()[still] + 1e-12).all()), name
        z = ((mean - want).abs() / (sd / math.sqrt(CALLS)))[~still]
        print(f'{activation} bits {bits} {name}: worst element {float(z.max()):.2f} standard errors')
        worst = max(worst, float(z.max()))
    assert worst <= 5.0


# ---- poisoned groups, constant groups, +-0 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bits', BITS)
def test_a_non_finite_element_poisons_its_group_of_its_own_part_only(bits):
    n = 200
    gate, up = draw(n)
    gate[70], up[5], up[199] = float('nan'), float('inf'), float('-inf')
    gq, uq = decoded(cabi_x.glu_state_host(gate, up, SEED, bits), n, bits)
    group = torch.arange(n) // 64
    assert torch.equal(torch.isnan(gq), group == 1) and torch.equal(torch.isnan(uq), (group == 0) | (group == 3))
    clean = cabi_x.glu_state_host(torch.nan_to_num(gate, 0.0), torch.nan_to_num(up, 0.0, 0.0, 0.0), SEED, bits)
    cg, cu = decoded(clean, n, bits)
    assert torch.equal(gq[group != 1], cg[group != 1]) and torch.equal(uq[group == 2], cu[group == 2])   # other groups: untouched to the bit


@pytest.mark.parametrize('bits', BITS)
def test_constant_groups_and_signed_zeros_decode_exactly(bits):
    n = 128
    gate = torch.cat((torch.full((64, ), 0.3), torch.zeros(64)))
    gate[64::3] = -0.0
    up = torch.cat((torch.zeros(64), torch.full((64, ), -1e-30)))
    gq, uq = decoded(cabi_x.glu_state_host(gate, up, SEED, bits), n, bits)
    assert torch.equal(gq[:64], gate[:64]) and bool((gq[64:] == 0).all()) and torch.equal(uq, up)
    assert not torch.signbit(gq[64:]).any()                         # lo = -0, step = +0: fma(code, +0, -0) = +0 + -0 = +0
    assert not torch.signbit(uq[:64]).any()


# ---- the node on host tensors ------------------------------------------------------------------------------------------------------------------------
def problem(shape=(3, 5, 48), dtype=torch.float32, salt=0):
    g = torch.Generator().manual_seed(23 + salt)
    return (torch.randn(*shape, generator=g).to(dtype).requires_grad_(), torch.randn(*shape, generator=g).to(dtype).requires_grad_(),
            torch.randn(*shape, generator=g).to(dtype))


@pytest.mark.parametrize('activation', ('silu', 'gelu'))
def test_nothing_of_the_inputs_shape_is_saved_but_the_codes_and_the_gradients_are_close(activation):
    gate, up, gy = problem()
    torch.manual_seed(3)
    y, saved = saved_by(lambda: fewbit.functional.glu_quantized(gate, up, activation, 8))
    exact = (F.silu(gate) if activation == 'silu' else F.gelu(gate)) * up
    assert torch.equal(y, exact.detach()) and type(y.grad_fn).__name__ == '_GLUQuantizedBackward'
    n = gate.numel()
    assert sorted(t.numel() for t in saved) == sorted(2 * [math.ceil(n / 64) * 64] + 4 * [math.ceil(n / 64)])
    assert all(t.dtype == torch.uint8 for t in saved if t.numel() >= n)
    d_gate, d_up = torch.autograd.grad(y, (gate, up), gy)
    e_gate, e_up = torch.autograd.grad(exact, (gate, up), gy)
    # 8 bits: the step is 1 / 255 of a group's range (about 5 here), an element is moved by at most one step
    assert float((d_up - e_up).abs().max()) <= 0.05 * float(gy.abs().max())
    assert float((d_gate - e_gate).abs().max()) <= 0.1 * float((gy * up.detach()).abs().max() + gy.abs().max())
    with pytest.raises(RuntimeError):                               # once_differentiable: no second derivative
        gg, = torch.autograd.grad(fewbit.functional.glu_quantized(gate, up, activation), gate, gy, create_graph=True)
        gg.sum().backward()


@pytest.mark.parametrize('bits', BITS)
def test_the_packed_form_gives_the_values_of_two_tensors_with_the_same_seed(bits):
    gate, up, gy = problem()
    packed = torch.cat((gate.detach(), up.detach()), dim=-1).requires_grad_()
    torch.manual_seed(11)
    y2 = fewbit.functional.glu_quantized(gate, up, 'silu', bits)
    g2 = torch.autograd.grad(y2, (gate, up), gy)
    torch.manual_seed(11)
    y1 = fewbit.functional.glu_quantized(packed, None, 'silu', bits)
    g1, = torch.autograd.grad(y1, packed, gy)
    assert torch.equal(y1, y2) and g1.shape == packed.shape and torch.equal(g1, torch.cat(g2, dim=-1))
    halves_of_a_view = packed.detach().chunk(2, dim=-1)
    torch.manual_seed(11)
    with torch.enable_grad():
        a, b = (t.requires_grad_() for t in (halves_of_a_view[0].clone(), halves_of_a_view[1].clone()))
        assert torch.equal(fewbit.functional.glu_quantized(a, b, 'silu', bits), y2)
    with pytest.raises(ValueError, match='even'):
        fewbit.functional.glu_quantized(torch.zeros(3, 5, requires_grad=True))
    with pytest.raises(ValueError, match='shape of gate'):
        fewbit.functional.glu_quantized(gate, up[:2])


def test_no_grad_a_frozen_input_eval_and_the_refusals(seeds):  # noqa: F811
    gate, up, gy = problem()
    layer = fewbit.QuantizedGLU('gelu', bits=4)
    exact = F.gelu(gate.detach()) * up.detach()
    y, saved = saved_by(lambda: layer(gate, up))
    assert len(seeds) == 0 and saved and torch.equal(y, exact)                      # (the host formulation draws from the generator, not a seed)
    state = torch.get_rng_state()
    with torch.no_grad():
        y, saved = saved_by(lambda: layer(gate, up))
    assert y.grad_fn is None and not saved and torch.equal(y, exact) and torch.equal(torch.get_rng_state(), state)
    y, saved = saved_by(lambda: layer(gate.detach(), up.detach()))
    assert y.grad_fn is None and not saved and torch.equal(torch.get_rng_state(), state)
    # one frozen input: the node, and no gradient for the frozen one
    y = layer(gate, up.detach())
    assert type(y.grad_fn).__name__ == '_GLUQuantizedBackward'
    d_gate, = torch.autograd.grad(y, gate, gy)
    assert d_gate.shape == gate.shape
    y = layer(gate.detach(), up)
    assert torch.autograd.grad(y, up, gy)[0].shape == up.shape
    # eval: torch's exact product and its exact gradients, nothing rounded or drawn
    layer.eval()
    state = torch.get_rng_state()
    y, saved = saved_by(lambda: layer(gate, up))
    assert 'GLUQuantized' not in type(y.grad_fn).__name__ and not any(t.dtype == torch.uint8 for t in saved) and torch.equal(torch.get_rng_state(), state)
    got = torch.autograd.grad(y, (gate, up), gy)
    want = torch.autograd.grad(F.gelu(gate) * up, (gate, up), gy)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    packed = torch.cat((gate.detach(), up.detach()), dim=-1).requires_grad_()
    assert torch.equal(layer(packed), exact)
    for make in (lambda: fewbit.QuantizedGLU(bits=3), lambda: fewbit.functional.glu_quantized(gate, up, bits=3), lambda: fewbit.QuantizedGatedMLP(4, 8, bits=3)):
        with pytest.raises(ValueError, match='bits should be 2, 4 or 8'):
            make()
    for make in (lambda: fewbit.QuantizedGLU('gelu_tanh'), lambda: fewbit.functional.glu_quantized(gate, up, 'relu')):
        with pytest.raises(ValueError, match="'silu' or 'gelu'"):
            make()
    assert 'bits=4' in repr(layer) and "'gelu'" in repr(layer)


@pytest.mark.parametrize('reentrant', (False, True))
def test_checkpointing_gives_the_plain_runs_bits(reentrant):
    gate, up, gy = problem(salt=2)
    call = lambda a, b: fewbit.functional.glu_quantized(a, b, 'silu', 4)
    torch.manual_seed(12)
    y0 = call(gate, up)
    plain = torch.autograd.grad(y0, (gate, up), gy)
    torch.manual_seed(12)
    y = checkpoint(call, gate, up, use_reentrant=reentrant)
    y.backward(gy)
    assert torch.equal(y, y0) and torch.equal(gate.grad, plain[0]) and torch.equal(up.grad, plain[1])


class StubMLP(torch.nn.Module):
    """the MLP of a Llama-style model, as such models spell it"""

    def __init__(self, act_fn, width=16, hidden=40):
        super().__init__()
        self.gate_proj = torch.nn.Linear(width, hidden, bias=False)
        self.up_proj = torch.nn.Linear(width, hidden, bias=False)
        self.down_proj = torch.nn.Linear(hidden, width, bias=False)
        self.act_fn = act_fn

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


class StubBlock(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.norm = torch.nn.LayerNorm(16)
        self.mlp = StubMLP(torch.nn.SiLU())

    def forward(self, x):
        return x + self.mlp(self.norm(x))


@pytest.mark.parametrize('act_fn,name', ((torch.nn.SiLU(), 'silu'), (torch.nn.GELU(), 'gelu'), (F.silu, 'silu'), (F.gelu, 'gelu')))
def test_from_mlp_shares_the_projections_of_a_stub(act_fn, name):
    torch.manual_seed(0)
    stub = StubMLP(act_fn)
    mlp = fewbit.QuantizedGatedMLP.from_mlp(stub, bits=8)
    assert mlp.glu.activation == name and mlp.glu.bits == 8 and mlp.training
    assert mlp.gate_proj.weight is stub.gate_proj.weight and mlp.up_proj.weight is stub.up_proj.weight and mlp.down_proj.weight is stub.down_proj.weight
    assert len(list(mlp.parameters())) == 3 and not any(p.is_meta for p in mlp.parameters())
    x = torch.randn(6, 16, requires_grad=True)
    y, saved = saved_by(lambda: mlp(x))
    assert torch.equal(y, stub(x)) and any(t.dtype == torch.uint8 for t in saved)
    got = torch.autograd.grad(y.sum(), stub.gate_proj.weight)[0]
    want = torch.autograd.grad(stub(x).sum(), stub.gate_proj.weight)[0]
    assert float((got - want).abs().max()) <= 0.05 * float(want.abs().max()) + 1e-3
    assert not fewbit.QuantizedGatedMLP.from_mlp(stub.eval()).training


def test_from_mlp_refuses_other_activations_and_other_modules():
    for act_fn in (torch.nn.GELU(approximate='tanh'), torch.nn.ReLU(), torch.tanh, lambda t: F.gelu(t, approximate='tanh')):
        with pytest.raises(ValueError, match='activation of a gated MLP'):
            fewbit.QuantizedGatedMLP.from_mlp(StubMLP(act_fn))
    with pytest.raises(TypeError, match='gate_proj'):
        fewbit.QuantizedGatedMLP.from_mlp(torch.nn.Linear(4, 4))


def test_map_module_swaps_the_mlp_of_a_llama_style_model():
    torch.manual_seed(1)
    model = torch.nn.Sequential(StubBlock(), StubBlock())
    x = torch.randn(7, 16)
    want = model(x)
    swap = lambda m, path: fewbit.QuantizedGatedMLP.from_mlp(m, bits=4) if type(m).__name__.endswith('MLP') else m
    model = fewbit.map_module(model, swap)
    assert all(type(block.mlp) is fewbit.QuantizedGatedMLP for block in model)
    y, saved = saved_by(lambda: model(x))
    assert torch.equal(y, want) and sum(t.dtype == torch.uint8 for t in saved) == 4
    y.sum().backward()
    assert all(p.grad is not None for p in model.parameters())
