"""``fewbit.functional.glu_quantized``, ``fewbit.QuantizedGLU`` and ``fewbit.QuantizedGatedMLP`` on the GPU: the node runs the kernels (one uint8
buffer of ``glu_state_bytes`` bytes is all it saves, and the recorded seed reproduces it on the host), the halves of ``x.chunk(2, -1)`` and the
packed ``[gate | up]`` form give the bytes of two dense tensors, and the layer behaves inside autocast, both checkpoint modes, no_grad / eval,
with the kernels switched off and on float64."""
import pytest
import torch
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

import fewbit
from fewbit_amd import cabi_x, linear
from norm_harness import DEV, native_sketch_on, saved_by, seeds  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

BITS = (2, 4, 8)


def problem(shape=(3, 5, 72), dtype=torch.bfloat16, salt=0):
    g = torch.Generator().manual_seed(61 + salt)
    return ((3 * torch.randn(*shape, generator=g)).to(dtype).to(DEV).requires_grad_(), (3 * torch.randn(*shape, generator=g)).to(dtype).to(DEV).requires_grad_(),
            torch.randn(*shape, generator=g).to(dtype).to(DEV))


def entry_points(gate, up, gy, activation, bits, seed):
    rows = gate.numel() // gate.shape[-1]
    y, state = cabi_x.glu_forward(gate.detach().reshape(rows, -1).contiguous(), up.detach().reshape(rows, -1).contiguous(), activation, bits, seed)
    d_gate, d_up = cabi_x.glu_backward(gy.reshape(rows, -1).contiguous(), state, activation, bits)
    return y.view(gate.shape), d_gate.view(gate.shape), d_up.view(gate.shape), state


@pytest.mark.parametrize('activation', ('silu', 'gelu'))
@pytest.mark.parametrize('dtype', (torch.float32, torch.float16, torch.bfloat16))
def test_the_functional_runs_the_kernels_and_saves_the_state_alone(dtype, activation, seeds):  # noqa: F811
    for bits in BITS:
        gate, up, gy = problem(dtype=dtype, salt=bits)
        y, saved = saved_by(lambda: fewbit.functional.glu_quantized(gate, up, activation, bits))
        assert type(y.grad_fn).__name__ == '_GLUQuantizedBackward' and y.dtype == dtype and y.shape == gate.shape
        assert len(saved) == 1 and saved[0].dtype == torch.uint8 and saved[0].numel() == cabi_x.glu_state_bytes(gate.numel(), bits)
        # the recorded seed reproduces the state on the host, and the gradients are the entry points'
        assert torch.equal(saved[0].cpu(), cabi_x.glu_state_host(gate.detach().float(), up.detach().float(), seeds[-1], bits))
        d_gate, d_up = torch.autograd.grad(y, (gate, up), gy)
        ye, dge, due, _ = entry_points(gate, up, gy, activation, bits, seeds[-1])
        assert torch.equal(y, ye) and torch.equal(d_gate, dge) and torch.equal(d_up, due)
    assert len(seeds) == len(BITS)


def test_the_module_and_the_gated_mlp(seeds):  # noqa: F811
    gate, up, gy = problem()
    layer = fewbit.QuantizedGLU('silu', bits=4)
    y = layer(gate, up)
    ye, dge, due, _ = entry_points(gate, up, gy, 'silu', 4, seeds[-1])
    got = torch.autograd.grad(y, (gate, up), gy)
    assert torch.equal(y, ye) and torch.equal(got[0], dge) and torch.equal(got[1], due)
    torch.manual_seed(0)
    mlp = fewbit.QuantizedGatedMLP(64, 176, activation='gelu', bits=8, device=DEV, dtype=torch.bfloat16)
    x = torch.randn(4, 9, 64, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    out, saved = saved_by(lambda: mlp(x))
    states = [t for t in saved if t.dtype == torch.uint8]
    assert len(states) == 1 and states[0].numel() == cabi_x.glu_state_bytes(4 * 9 * 176, 8)
    # of the intermediate width only the product itself is kept (by down_proj, for its weight gradient): not gate, act(gate) or up
    assert sum(t.dtype == torch.bfloat16 and t.numel() == 4 * 9 * 176 for t in saved) == 1
    exact = mlp.down_proj(F.gelu(mlp.gate_proj(x).float()).mul(mlp.up_proj(x).float()).bfloat16())
    assert float((out.detach().float() - exact.detach().float()).abs().max()) <= 2.0**-6 * float(exact.detach().float().abs().max())
    out.float().sum().backward()
    want = torch.autograd.grad(exact.float().sum(), mlp.gate_proj.weight)[0]
    assert float((mlp.gate_proj.weight.grad.float() - want.float()).norm()) <= 0.1 * float(want.float().norm())


@pytest.mark.parametrize('bits', BITS)
def test_chunk_views_and_the_packed_form_give_the_bytes_of_two_dense_tensors(bits, seeds):  # noqa: F811
    gate, up, gy = problem((4, 7, 72), salt=3)
    torch.manual_seed(5)
    y0 = fewbit.functional.glu_quantized(gate, up, 'silu', bits)
    g0 = torch.autograd.grad(y0, (gate, up), gy)
    packed = torch.cat((gate.detach(), up.detach()), dim=-1).requires_grad_()
    a, b = packed.chunk(2, dim=-1)                                    # views with row stride 144: taken as they are
    torch.manual_seed(5)
    y1, saved = saved_by(lambda: fewbit.functional.glu_quantized(a, b, 'silu', bits))
    g1, = torch.autograd.grad(y1, packed, gy)
    assert torch.equal(y1, y0) and torch.equal(g1, torch.cat(g0, dim=-1)) and len(saved) == 1
    torch.manual_seed(5)
    y2 = fewbit.functional.glu_quantized(packed, None, 'silu', bits)
    g2, = torch.autograd.grad(y2, packed, gy)
    assert torch.equal(y2, y0) and g2.shape == packed.shape and g2.is_contiguous() and torch.equal(g2, g1)
    assert seeds[0] == seeds[1] == seeds[2]
    # a layout with no single row stride is gathered first
    wide = torch.randn(4, 7, 144, device=DEV).bfloat16()
    t = wide[:, ::2, :72].transpose(0, 1)
    torch.manual_seed(5)
    y3 = fewbit.functional.glu_quantized(t.requires_grad_(), t, 'silu', bits)
    torch.manual_seed(5)
    dense = t.detach().contiguous().requires_grad_()
    assert torch.equal(y3, fewbit.functional.glu_quantized(dense, dense, 'silu', bits))


def test_backward_may_follow_the_autocast_block(seeds):  # noqa: F811
    torch.manual_seed(2)
    mlp = fewbit.QuantizedGatedMLP(64, 128, device=DEV)             # fp32 parameters
    x = torch.randn(6, 64, device=DEV, requires_grad=True)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        gate, up = mlp.gate_proj(x), mlp.up_proj(x)
        h, saved = saved_by(lambda: mlp.glu(gate, up))
        out = mlp.down_proj(h)
    assert h.dtype == torch.bfloat16 and type(h.grad_fn).__name__ == '_GLUQuantizedBackward' and len(saved) == 1
    gy = torch.randn_like(h)
    d_gate, d_up = torch.autograd.grad(h, (gate, up), gy, retain_graph=True)      # outside the block: the ordinary AMP pattern
    ye, dge, due, _ = entry_points(gate, up, gy, 'silu', 4, seeds[0])
    assert torch.equal(h, ye) and torch.equal(d_gate, dge) and torch.equal(d_up, due) and d_gate.dtype == torch.bfloat16
    out.float().sum().backward()
    assert x.grad is not None and mlp.gate_proj.weight.grad.dtype == torch.float32


@pytest.mark.parametrize('reentrant', (False, True))
def test_checkpointing_gives_the_plain_runs_bits(reentrant):
    gate, up, gy = problem(salt=2)
    call = lambda a, b: fewbit.functional.glu_quantized(a, b, 'gelu', 4)
    torch.manual_seed(12)
    y0 = call(gate, up)
    plain = torch.autograd.grad(y0, (gate, up), gy)
    torch.manual_seed(12)
    y = checkpoint(call, gate, up, use_reentrant=reentrant)
    y.backward(gy)
    assert torch.equal(y, y0) and torch.equal(gate.grad, plain[0]) and torch.equal(up.grad, plain[1])


def test_no_grad_eval_and_frozen_inputs_keep_nothing_and_draw_nothing(seeds):  # noqa: F811
    gate, up, gy = problem()
    layer = fewbit.QuantizedGLU('silu', bits=4)
    y_train, _ = saved_by(lambda: layer(gate, up))
    assert len(seeds) == 1
    with torch.no_grad():
        y, saved = saved_by(lambda: layer(gate, up))
    assert y.grad_fn is None and not saved and torch.equal(y, y_train)               # the plain forward: the same bytes
    y, saved = saved_by(lambda: layer(gate.detach(), up.detach()))
    assert y.grad_fn is None and not saved and torch.equal(y, y_train)
    with torch.inference_mode():
        assert torch.equal(layer(gate, up), y_train)
    packed = torch.cat((gate.detach(), up.detach()), dim=-1)
    assert torch.equal(layer(packed), y_train) and len(seeds) == 1
    layer.eval()
    y, saved = saved_by(lambda: layer(gate, up))
    assert 'GLUQuantized' not in type(y.grad_fn).__name__ and not any(t.dtype == torch.uint8 for t in saved) and len(seeds) == 1
    want = torch.autograd.grad(F.silu(gate) * up, (gate, up), gy)
    assert all(torch.equal(a, b) for a, b in zip(torch.autograd.grad(y, (gate, up), gy), want))
    with torch.no_grad():
        assert torch.equal(layer(gate, up), y_train)
    layer.train()
    y = layer(gate, up.detach())                                                       # one frozen input: its gradient is not computed
    d_gate, = torch.autograd.grad(y, gate, gy)
    _, dge, _, _ = entry_points(gate, up, gy, 'silu', 4, seeds[-1])
    assert torch.equal(d_gate, dge)
    with pytest.raises(ValueError, match='bits should be 2, 4 or 8'):
        fewbit.functional.glu_quantized(gate, up, bits=3)


def test_the_switch_and_float64_take_the_pytorch_formulation(seeds):  # noqa: F811
    gate, up, gy = problem(dtype=torch.float32)
    linear.use_native_sketch(False)
    y, saved = saved_by(lambda: fewbit.functional.glu_quantized(gate, up, 'silu', 8))
    assert len(seeds) == 0 and len(saved) == 6 and torch.equal(y, (F.silu(gate) * up).detach())
    d_gate, d_up = torch.autograd.grad(y, (gate, up), gy)
    e_gate, e_up = torch.autograd.grad(F.silu(gate) * up, (gate, up), gy)
    # (8 bits: an element moves by at most a step, 1 / 255 of a group's range of about 18)
    assert float((d_up - e_up).norm()) <= 0.05 * float(e_up.norm()) and float((d_gate - e_gate).norm()) <= 0.05 * float(e_gate.norm())
    linear.use_native_sketch(True)
    g64, u64 = gate.detach().double().requires_grad_(), up.detach().double().requires_grad_()
    y, saved = saved_by(lambda: fewbit.functional.glu_quantized(g64, u64, 'gelu', 8))
    assert len(seeds) == 0 and y.dtype == torch.float64 and torch.equal(y, (F.gelu(g64) * u64).detach())
    d_gate, d_up = torch.autograd.grad(y, (g64, u64), gy.double())
    e_gate, e_up = torch.autograd.grad(F.gelu(g64) * u64, (g64, u64), gy.double())
    assert d_gate.dtype == torch.float64 and float((d_up - e_up).norm()) <= 0.05 * float(e_up.norm()) and float((d_gate - e_gate).norm()) <= 0.05 * float(e_gate.norm())
