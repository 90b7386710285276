"""``fewbit.functional.gated_mlp_quantized`` and ``fewbit.QuantizedGatedMLP(fused=True)`` on the GPU: the node is, bit for bit, the composition of the
entry points it stands for (``quant_pack``, ``glu_forward``, ``glu_backward_product``, ``quant_unpack`` and torch's GEMMs in the node's order) for the
two seeds it drew; it saves the two states and the weights and nothing else; at 8 bits its gradients are no further from float64 than those of the
layers it replaces; and it behaves inside autocast, no_grad, eval, with frozen projections and in a captured graph."""
import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi, cabi_x, linear
from gated_mlp_harness import exact_mlp, parameters_of
from norm_harness import DEV, native_sketch_on, saved_by, seeds  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

BITS = (2, 4, 8)
SHAPE, H = (2, 12, 40), 40                                          # T = 24 tokens
HIDDEN = (72, 100)                                                  # the vector path; the element path (100 is no multiple of 8)
MAX_SLOPE = 1.13                                                    # |act'| <= 1.0999 (silu), 1.1290 (gelu)


def problem(hidden, dtype, bias=True, bits=4, activation='silu', salt=0, fused=True):
    torch.manual_seed(31 + salt)
    mlp = fewbit.QuantizedGatedMLP(H, hidden, bias=bias, activation=activation, bits=bits, device=DEV, dtype=dtype, fused=fused)
    g = torch.Generator().manual_seed(47 + salt)
    x = (2 * torch.randn(*SHAPE, generator=g)).to(dtype).to(DEV).requires_grad_()
    return mlp, x, torch.randn(*SHAPE, generator=g).to(dtype).to(DEV)


def composed(mlp, x, gy, activation, bits, seed_x, seed_gu):
    """-> (out, {name: gradient}) from the entry points and torch's GEMMs, in the order of the node"""
    Wg, Wu, Wd, bg, bu, bd = (t if t is None else t.detach() for t in (mlp.gate_proj.weight, mlp.up_proj.weight, mlp.down_proj.weight, mlp.gate_proj.bias,
                                                                      mlp.up_proj.bias, mlp.down_proj.bias))
    x = x.detach()
    flat = x.reshape(-1, x.shape[-1]).contiguous()
    rows, hidden = flat.shape[0], Wg.shape[0]
    state_x = cabi_x.quant_pack(flat, seed_x, bits)
    gate, up = F.linear(x, Wg, bg).reshape(rows, hidden), F.linear(x, Wu, bu).reshape(rows, hidden)
    y, state = cabi_x.glu_forward(gate, up, activation, bits, seed_gu)
    out = F.linear(y.view(*x.shape[:-1], hidden), Wd, bd)
    G = gy.reshape(rows, -1)
    both = torch.empty(rows, 2 * hidden, dtype=G.dtype, device=G.device)
    product = torch.empty(rows, hidden, dtype=G.dtype, device=G.device)
    d_gate, d_up, _ = cabi_x.glu_backward_product(G @ Wd, state, activation, bits, (True, True, True), both[:, :hidden], both[:, hidden:], product)
    grads = {'down_proj.weight': G.T @ product, 'down_proj.bias': G.sum(dim=0), 'gate_proj.bias': d_gate.sum(dim=0), 'up_proj.bias': d_up.sum(dim=0)}
    if linear._decode_in_two_terms(bits, G.dtype):
        decoded = cabi_x.quant_unpack(state_x, flat.numel(), bits, torch.float32).view(flat.shape)
        grads['gate_proj.weight'] = linear._two_term_product(d_gate, decoded).to(G.dtype)
        grads['up_proj.weight'] = linear._two_term_product(d_up, decoded).to(G.dtype)
    else:
        decoded = cabi_x.quant_unpack(state_x, flat.numel(), bits, G.dtype).view(flat.shape)
        grads['gate_proj.weight'], grads['up_proj.weight'] = d_gate.T @ decoded, d_up.T @ decoded
    grads['x'] = torch.addmm(d_gate @ Wg, d_up, Wu).view(x.shape)
    return out, grads, (state_x, state)


# ---- against the composition ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('activation', ('silu', 'gelu'))
@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float32))
@pytest.mark.parametrize('hidden', HIDDEN)
def test_the_node_is_the_composition_of_the_entry_points(hidden, dtype, activation, seeds):  # noqa: F811
    for bits in BITS:
        mlp, x, gy = problem(hidden, dtype, bits=bits, activation=activation, salt=bits)
        out, saved = saved_by(lambda: mlp(x))
        assert type(out.grad_fn).__name__ == '_GatedMLPQuantizedBackward' and out.dtype == dtype and out.shape == x.shape
        assert len(seeds) >= 2
        seed_x, seed_gu = seeds[-2], seeds[-1]
        names, leaves = zip(*([('x', x)] + parameters_of(mlp)))
        got = dict(zip(names, torch.autograd.grad(out, leaves, gy)))
        want_out, want, states = composed(mlp, x, gy, activation, bits, seed_x, seed_gu)
        assert torch.equal(out, want_out)
        kept = [t for t in saved if t.dtype == torch.uint8]
        assert len(kept) == 2 and torch.equal(kept[0], states[0]) and torch.equal(kept[1], states[1])
        for name in names:
            assert got[name].dtype == want[name].dtype and torch.equal(got[name], want[name]), (name, bits)
    assert len(seeds) == 2 * len(BITS)                               # two draws per call: the seed of x first


# ---- saved bytes ---------------------------------------------------------------------------------------------------------------------------------------
def unique_bytes(saved):
    """bytes of what the saved tensors hold, every storage counted once (torch's linear saves views of x and of its weight)"""
    return sum({t.untyped_storage().data_ptr(): t.untyped_storage().nbytes() for t in saved}.values())


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('hidden', HIDDEN)
def test_the_saved_bytes_are_the_two_states_and_the_weights(hidden, bits):
    dtype, rows = torch.bfloat16, 24
    mlp, x, _ = problem(hidden, dtype, bias=False, bits=bits)
    weights = 3 * H * hidden * 2
    out, saved = saved_by(lambda: mlp(x))
    assert len(saved) == 5
    assert unique_bytes(saved) == cabi_x.quant_bytes(rows * H, bits) + cabi_x.glu_state_bytes(rows * hidden, bits) + weights
    assert not any(t.is_floating_point() and t.numel() in (rows * H, rows * hidden) for t in saved)
    # the layers it replaces keep x and the product y in full as well
    mlp.fused = False
    out2, saved2 = saved_by(lambda: mlp(x))
    assert torch.equal(out, out2)
    assert unique_bytes(saved2) == rows * H * 2 + cabi_x.glu_state_bytes(rows * hidden, bits) + rows * hidden * 2 + weights
    assert unique_bytes(saved2) - unique_bytes(saved) == rows * H * 2 + rows * hidden * 2 - cabi_x.quant_bytes(rows * H, bits)


# ---- the error of the gradients at 8 bits ----------------------------------------------------------------------------------------------------------------
class ThreeQuantizedLinears(torch.nn.Module):
    """the exact product between three ``QuantizedLinear`` layers that share the projections' parameters: the error of keeping x and y in 8 bits alone"""

    def __init__(self, mlp, bits):
        super().__init__()
        self.gate, self.up, self.down = (fewbit.QuantizedLinear.from_linear(m, bits=bits) for m in (mlp.gate_proj, mlp.up_proj, mlp.down_proj))
        self.activation = mlp.glu.activation

    def forward(self, x):
        gate = self.gate(x)
        return self.down((F.silu(gate) if self.activation == 'silu' else F.gelu(gate)) * self.up(x))


@pytest.mark.parametrize('activation', ('silu', 'gelu'))
@pytest.mark.parametrize('hidden', HIDDEN)
def test_the_gradients_at_8_bits_are_no_further_from_float64_than_those_of_the_layers_replaced(hidden, activation):
    """fp32, 8 bits.  The relative error (in norm) of every gradient against the float64 gradients of the exact MLP is at most that of the unfused module
    with the same state of gate and up (the same seed: one draw is spent first, where the node draws the seed of x) plus that of three
    ``QuantizedLinear`` layers at 8 bits around the exact product: what the node adds to the former is x^ for x and y^ for y, the latter's errors.

    MEASURED on an MI355X (silu, I = 72; fused / unfused / three QuantizedLinear): dx 8.89e-3 / 8.89e-3 / 2.6e-7 and the two bias gradients of gate and up
    likewise equal to the unfused module's (the same d_gate and d_up); gate_proj.weight 1.16e-2 / 9.3e-3 / 6.8e-3; up_proj.weight 1.00e-2 / 7.5e-3 / 7.0e-3;
    down_proj.weight 1.04e-2 / 2.4e-7 / 1.18e-2 (I = 100: 1.14e-2 against 1.19e-2): y^ = act(g^) u^ is no worse a stand-in for y than y kept in 8 bits."""
    bits = 8
    mlp, x, gy = problem(hidden, torch.float32, bits=bits, activation=activation, salt=5)
    names, leaves = zip(*([('x', x)] + parameters_of(mlp)))
    reference = fewbit.QuantizedGatedMLP(H, hidden, bias=True, activation=activation, dtype=torch.float64, device=DEV)
    reference.load_state_dict({k: v.double() for k, v in mlp.state_dict().items()})
    x64 = x.detach().double().requires_grad_()
    exact = torch.autograd.grad(exact_mlp(x64, reference, activation), [x64] + [p for _, p in parameters_of(reference)], gy.double())

    def errors(module, spend=0):
        torch.manual_seed(77)
        for _ in range(spend):
            linear._draw_seed(None)
        grads = torch.autograd.grad(module(x), leaves, gy)
        return {name: float((g.double() - e).norm() / e.norm()) for name, g, e in zip(names, grads, exact)}

    fused = errors(mlp)
    mlp.fused = False
    unfused = errors(mlp, spend=1)
    quantized = errors(ThreeQuantizedLinears(mlp, bits))
    for name in names:
        print(f'{activation} I = {hidden} {name}: fused {fused[name]:.3e}, unfused {unfused[name]:.3e}, three QuantizedLinear {quantized[name]:.3e}')
    for name in names:
        assert fused[name] <= unfused[name] + quantized[name], name


# ---- wrappers and modes ----------------------------------------------------------------------------------------------------------------------------------
def test_backward_may_follow_the_autocast_block(seeds):  # noqa: F811
    mlp, x, gy = problem(72, torch.float32, bits=8)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out, saved = saved_by(lambda: mlp(x))
    assert out.dtype == torch.bfloat16 and type(out.grad_fn).__name__ == '_GatedMLPQuantizedBackward' and len(seeds) == 2
    kept = [t for t in saved if t.dtype == torch.uint8]
    assert [t.numel() for t in kept] == [cabi_x.quant_bytes(24 * H, 8), cabi_x.glu_state_bytes(24 * 72, 8)]
    names, leaves = zip(*([('x', x)] + parameters_of(mlp)))
    got = torch.autograd.grad(out, leaves, gy.bfloat16())           # outside the block: the ordinary AMP pattern
    want = torch.autograd.grad(exact_mlp(x, mlp, 'silu'), leaves, gy.bfloat16().float())
    for name, a, b in zip(names, got, want):
        assert a.dtype == torch.float32 and a.shape == b.shape, name
        # (bf16 GEMMs on bf16 operands and 8-bit states: the allowance test_gpu_glu_layer.py gives the unfused module for the same)
        assert float((a - b).norm()) <= 0.1 * float(b.norm()), name


def test_no_grad_eval_and_frozen_projections_keep_nothing_they_do_not_need(seeds):  # noqa: F811
    mlp, x, gy = problem(72, torch.bfloat16)
    trained, saved = saved_by(lambda: mlp(x))
    assert len(seeds) == 2 and sum(t.dtype == torch.uint8 for t in saved) == 2
    with torch.no_grad():
        out, saved = saved_by(lambda: mlp(x))
    assert out.grad_fn is None and not saved and torch.equal(out, trained)          # the plain forward: the same bytes
    with torch.inference_mode():
        assert torch.equal(mlp(x), trained)
    mlp.eval()
    out, saved = saved_by(lambda: mlp(x))
    assert 'GatedMLPQuantized' not in type(out.grad_fn).__name__ and not any(t.dtype == torch.uint8 for t in saved)
    leaves = [x] + [p for _, p in parameters_of(mlp)]
    assert all(torch.equal(a, b) for a, b in zip(torch.autograd.grad(out, leaves, gy), torch.autograd.grad(exact_mlp(x, mlp, 'silu'), leaves, gy)))
    with torch.no_grad():
        assert torch.equal(mlp(x), trained)
    assert len(seeds) == 2
    mlp.train()
    # frozen gate_proj and up_proj: no x^ is kept; the other gradients are the composition's
    mlp.gate_proj.requires_grad_(False)
    mlp.up_proj.requires_grad_(False)
    out, saved = saved_by(lambda: mlp(x))
    kept = [t for t in saved if t.dtype == torch.uint8]
    assert len(kept) == 1 and kept[0].numel() == cabi_x.glu_state_bytes(24 * 72, 4) and len(seeds) == 4
    got = torch.autograd.grad(out, (x, mlp.down_proj.weight, mlp.down_proj.bias), gy)
    want_out, want, _ = composed(mlp, x, gy, 'silu', 4, seeds[-2], seeds[-1])
    assert torch.equal(out, want_out) and torch.equal(out, trained)
    assert all(torch.equal(a, want[name]) for a, name in zip(got, ('x', 'down_proj.weight', 'down_proj.bias')))
    # everything frozen: the plain forward
    mlp.requires_grad_(False)
    out, saved = saved_by(lambda: mlp(x.detach()))
    assert out.grad_fn is None and not saved and torch.equal(out, trained) and len(seeds) == 4
    # down_proj's bias alone: a column sum of the incoming gradient -- nothing is rounded, nothing kept but the weights, no seed drawn
    mlp.down_proj.bias.requires_grad_(True)
    out, saved = saved_by(lambda: mlp(x.detach()))
    assert type(out.grad_fn).__name__ == '_GatedMLPQuantizedBackward' and len(saved) == 3 and not any(t.dtype == torch.uint8 for t in saved)
    assert torch.equal(out, trained) and len(seeds) == 4
    assert torch.equal(torch.autograd.grad(out, mlp.down_proj.bias, gy)[0], gy.reshape(-1, H).sum(dim=0))
    mlp.down_proj.bias.requires_grad_(False)
    # down_proj's weight alone: the state of gate and up, no x^, no gy for the kernel
    mlp.down_proj.weight.requires_grad_(True)
    out, saved = saved_by(lambda: mlp(x.detach()))
    assert sum(t.dtype == torch.uint8 for t in saved) == 1
    got, = torch.autograd.grad(out, mlp.down_proj.weight, gy)
    _, want, _ = composed(mlp, x, gy, 'silu', 4, seeds[-2], seeds[-1])
    assert torch.equal(got, want['down_proj.weight'])


def test_the_switch_and_float64_take_the_pytorch_formulation(seeds):  # noqa: F811
    mlp, x, gy = problem(72, torch.float32, bits=8)
    leaves = [x] + [p for _, p in parameters_of(mlp)]
    linear.use_native_sketch(False)
    out, saved = saved_by(lambda: mlp(x))
    assert len(seeds) == 0 and len(saved) == 12 and torch.equal(out, exact_mlp(x, mlp, 'silu').detach())
    got = torch.autograd.grad(out, leaves, gy)
    want = torch.autograd.grad(exact_mlp(x, mlp, 'silu'), leaves, gy)
    assert all(float((a - b).norm()) <= 0.05 * float(b.norm()) for a, b in zip(got, want))
    linear.use_native_sketch(True)
    mlp = mlp.double()
    x64 = x.detach().double().requires_grad_()
    out, saved = saved_by(lambda: mlp(x64))
    assert len(seeds) == 0 and out.dtype == torch.float64 and len(saved) == 12


# ---- a captured forward + backward --------------------------------------------------------------------------------------------------------------------------
def test_a_captured_forward_and_backward_round_afresh_on_every_replay(monkeypatch):
    """Three replays: three different gradients of down_proj's weight, each the composition's for the two seeds that replay's counter values give, and
    each within the band ANY rounding stays in: an element of g^ or u^ lies within a step of its value, so
    |act(g^) u^ - act(g) u| <= max|act'| step_g (|u| + step_u) + |act(g)| step_u, and the gradient moves by at most |G|^T of that."""
    bits, hidden = 4, 72
    mlp, x, gy = problem(hidden, torch.float32, bits=bits, salt=9)
    names, leaves = zip(*([('x', x)] + parameters_of(mlp)))

    def step():
        out = mlp(x)
        return (out, ) + torch.autograd.grad(out, leaves, gy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                        # the eager warm-up: the per-device replay counter exists from here on
    torch.cuda.current_stream().wait_stream(side)
    bases = []
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: bases.append(0x2468ace + len(bases)) or bases[-1])
    counter = linear._replay_counter(torch.device(DEV))
    torch.cuda.synchronize()
    c0 = int(counter)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, *grads = step()
    assert len(bases) == 2 and int(counter) == c0
    # the band, in float64 on the host
    with torch.no_grad():
        flat = x.detach().double().reshape(24, H).cpu()
        p = {k: v.double().cpu() for k, v in mlp.state_dict().items()}
        gate = flat @ p['gate_proj.weight'].T + p['gate_proj.bias']
        up = flat @ p['up_proj.weight'].T + p['up_proj.bias']
        act = gate * torch.sigmoid(gate)
        spread = lambda t: ((t.reshape(-1, 64).amax(dim=1) - t.reshape(-1, 64).amin(dim=1)) / (2**bits - 1)).repeat_interleave(64).view(t.shape)
        step_g, step_u = spread(gate), spread(up)
        moved = MAX_SLOPE * step_g * (up.abs() + step_u) + act.abs() * step_u
        G = gy.double().reshape(24, H).cpu()
        exact = G.T @ (act * up)
        band = G.abs().T @ moved + 1e-5 * (G.abs().T @ (act * up).abs())          # (fp32 GEMMs and the fp32 product beside the rounding)
    seen = []
    for replay in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert int(counter) == c0 + 2 * (replay + 1)
        seed_x, seed_gu = cabi.mix_sketch_seed(bases[0], c0 + 2 * replay), cabi.mix_sketch_seed(bases[1], c0 + 2 * replay + 1)
        want_out, want, _ = composed(mlp, x, gy, 'silu', bits, seed_x, seed_gu)
        assert torch.equal(out, want_out)
        for name, got in zip(names, grads):
            assert torch.equal(got, want[name]), (name, replay)
        dWd = grads[names.index('down_proj.weight')]
        assert bool(((dWd.double().cpu() - exact).abs() <= band).all())
        seen.append(dWd.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and not torch.equal(seen[0], seen[2])
