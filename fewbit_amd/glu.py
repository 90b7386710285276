"""The product of a gated MLP, ``act(gate) * up``, that keeps its two inputs in 2, 4 or 8 bits per element for backward.

``down(act(gate(x)) * up(x))`` is the MLP of the Llama / Mistral / Qwen / Gemma / T5-v1.1 family.  For the product torch saves ``gate``, ``act(gate)``
and ``up``: three tensors of the intermediate width, the largest thing such a block keeps.  Here ONE node keeps ``gate`` and ``up`` in the packed
form of a seed (include/fewbit_hipx.h, "the gate and the up of a seed": per 64 elements a minimum and a step, per element a code rounded
stochastically and without bias, the two tensors rounded with two independent streams of one seed) and nothing else: at 4 bits 0.3125 of the
bytes of the two bf16 inputs, a tenth of what torch keeps.  The few-bit activations of this package do not serve here: they keep a code for
``act'`` only, and the product also needs ``act(gate)`` and ``up`` themselves.

* The forward value is ``act(gate) * up`` with ``act`` in fp32 and ONE product, rounded once (torch rounds ``act(gate)`` to the dtype first, so a
  16-bit output may differ from torch's in its last bit).  Only the gradients see the rounding: ``d_up = gy * act(g^)`` and
  ``d_gate = gy * u^ * act'(g^)`` on the decodes ``g^``, ``u^``.  ``E[g^] = g`` and ``E[u^] = u``, but ``act`` is not linear: both gradients carry
  a bias of second order in the step (tests/test_glu_host.py checks the mean of many seeds against the exact expectation).
* The kernels (fewbit_amd/csrc/fewbit_glu.hip: one launch forward, one backward) serve fp32 / fp16 / bf16 GPU tensors while
  ``linear.use_native_sketch()`` is on.  ``gate`` and ``up`` may be two tensors -- any views with unit last stride and one row stride, such as
  the halves of ``x.chunk(2, -1)``, are taken as they are; other layouts are gathered first -- or ONE tensor ``[gate | up]`` along the last
  dimension (``up=None``), whose one gradient tensor the one backward launch then writes in place, without a copy.  Host tensors, float64 and
  ``use_native_sketch(False)`` take a PyTorch formulation of the same definition: ``y`` is torch's ``act(gate) * up``, the codes come from
  ``kept.quantize_groups``, backward is the formula above.
* ``activation``: ``'silu'`` or ``'gelu'`` (the erf form; the tanh form is not done).
* The seed comes from ``linear._sketch_seed``: an int drawn from the host generator, or a device word while the stream is being captured into a
  hipGraph (one eager call on the device precedes a capture, as for the randomized linears).
* With grad mode off, or when neither input requires grad, the call is the plain forward: no seed is drawn, nothing is kept, no node is built;
  on the kernel path ``y`` has the bytes of the keeping call.  A module in ``eval()`` mode gives torch's exact ``act(gate) * up`` where gradients
  are asked for.
* Backward runs under the autocast state the forward saw (``linear._autocast_as``).  Inside ``torch.utils.checkpoint`` the generator must be a
  default one (``generator=None`` included): checkpoint restores only those, and the recomputation must draw the forward's seed again.
* A group of 64 elements of either input that holds a NaN or an infinity makes both gradients NaN on those 64 elements; ``y`` is the exact forward.
* Not differentiable twice (``once_differentiable``).
"""
import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import cabi_x, kept, linear
from .cabi import DTYPES

__all__ = ('glu_quantized', 'gated_mlp_quantized', 'QuantizedGLU', 'QuantizedGatedMLP')

ACTIVATIONS = cabi_x.GLU_ACTIVATIONS


def _torch_product(gate: torch.Tensor, up: torch.Tensor, activation: str) -> torch.Tensor:
    """torch's own product (on dense tensors: its host kernels take another route through a strided half of ``[gate | up]``, and the last bit of the
    activation would then depend on the layout)"""
    gate, up = gate.contiguous(), up.contiguous()
    return (F.silu(gate) if activation == 'silu' else F.gelu(gate)) * up


def _halves(packed: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    if packed.dim() == 0 or packed.shape[-1] % 2:
        raise ValueError(f'the last dimension of [gate | up] should be even, but the shape is {tuple(packed.shape)}.')
    return packed.chunk(2, dim=-1)


def _rows(t: torch.Tensor) -> torch.Tensor:
    """``t`` (..., width) as a 2-D ``rows x width`` tensor the kernels take: a view where the last stride is 1 and ONE stride steps through all the
    rows (a contiguous tensor, a half of ``x.chunk(2, -1)``, a slice of the columns), a contiguous copy otherwise"""
    width = t.shape[-1]
    lead = [(n, s) for n, s in zip(t.shape[:-1], t.stride()[:-1]) if n != 1]
    rows = math.prod(n for n, _ in lead)
    if width == 1 or t.stride(-1) == 1:
        ld = lead[-1][1] if lead else width
        if ld >= width and all(s == n1 * s1 for (_, s), (n1, s1) in zip(lead, lead[1:])):
            return t.as_strided((rows, width), (ld, 1))
    return t.reshape(rows, width).contiguous()


def _kernel_applies(gate: torch.Tensor, up: torch.Tensor) -> bool:
    return linear._kernels_take(gate) and up.dtype == gate.dtype and up.device == gate.device


def _slope(g: torch.Tensor, activation: str) -> torch.Tensor:
    """``act'`` of the definition: silu ``s (1 + g (1 - s))``, gelu ``Phi(g) + g phi(g)``"""
    if activation == 'silu':
        s = torch.sigmoid(g)
        return s * (1 + g * (1 - s))
    return 0.5 * (1 + torch.erf(g * math.sqrt(0.5))) + g * torch.exp(-0.5 * g * g) * (1 / math.sqrt(2 * math.pi))


def _check(activation: str, bits: int) -> None:
    kept.check_bits(bits)
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation should be 'silu' or 'gelu', but got {activation!r}.")


def _formula_backward(gy: Optional[torch.Tensor], gate_kept, up_kept, shape, activation: str, want):
    """The PyTorch formulation of backward from the codes, lo and step of gate and of up -> ``(d_gate, d_up, product)`` in the dtype of the decodes,
    None where ``want`` is False: the definition's formulas on the decodes, NaN on the elements of a poisoned group"""
    count = math.prod(shape)
    g, u = kept.decode(*gate_kept, 1, count).view(shape), kept.decode(*up_kept, 1, count).view(shape)
    poisoned = torch.isnan(g) | torch.isnan(u)
    nan = torch.full((), float('nan'), dtype=g.dtype, device=g.device)
    if gy is not None:
        gy = gy.to(g.dtype)
    act = (F.silu(g) if activation == 'silu' else F.gelu(g)) if want[1] or want[2] else None
    d_gate = torch.where(poisoned, nan, gy * u * _slope(g, activation)) if want[0] else None
    d_up = torch.where(poisoned, nan, gy * act) if want[1] else None
    product = torch.where(poisoned, nan, act * u) if want[2] else None
    return d_gate, d_up, product


class _GLUQuantized(torch.autograd.Function):
    """``act(gate) * up`` that keeps both inputs in ``bits`` bits per element (module docstring).  ``up is None``: ``gate`` is ``[gate | up]``.  Kept for
    backward on the kernels: ONE uint8 buffer (the state); in the PyTorch formulation the codes (one per byte), lo and step of every group of both
    inputs.  On ``ctx``: the seed (an int; a device word while the stream is being captured)."""

    @staticmethod
    def forward(ctx, gate, up, activation: str, bits: int, generator):
        ctx.packed = up is None
        ctx.input_shape, ctx.input_dtype = tuple(gate.shape), gate.dtype
        g, u = _halves(gate.detach()) if ctx.packed else (gate.detach(), up.detach())
        ctx.activation, ctx.bits, ctx.shape, ctx.up_dtype = activation, bits, tuple(g.shape), u.dtype
        ctx.autocast = linear._autocast_seen(gate.device.type)
        ctx.native_seed = None
        if _kernel_applies(g, u):
            ctx.native_seed = linear._sketch_seed(generator, g.device)
            y, state = cabi_x.glu_forward(_rows(g), _rows(u), activation, bits, ctx.native_seed)
            ctx.save_for_backward(state)
            return y.view(ctx.shape)
        ctx.save_for_backward(*kept.quantize_groups(g, bits, generator), *kept.quantize_groups(u, bits, generator))
        return _torch_product(g, u, activation)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        with linear._autocast_as(ctx.autocast):
            grad_output = linear._dense_rows(grad_output)
            saved = ctx.saved_tensors                       # read once: a non-re-entrant checkpoint unpacks a saved tensor one time only
            width = ctx.shape[-1]
            want = (True, True) if ctx.packed else tuple(ctx.needs_input_grad[:2])
            if ctx.native_seed is None:
                d_gate, d_up, _ = _formula_backward(grad_output, saved[:3], saved[3:], ctx.shape, ctx.activation, (*want, False))
                if ctx.packed:
                    return torch.cat((d_gate, d_up), dim=-1).to(ctx.input_dtype), None, None, None, None
                return (None if d_gate is None else d_gate.to(ctx.input_dtype), None if d_up is None else d_up.to(ctx.up_dtype), None, None, None)
            gy = grad_output.reshape(-1, width)
            gy = gy if gy.dtype in DTYPES else gy.float()
            if ctx.packed:
                # ONE gradient tensor of the packed shape: the launch writes its two halves where they lie (row stride 2 width), no copy follows
                both = torch.empty((gy.shape[0], 2 * width), dtype=gy.dtype, device=gy.device)
                cabi_x.glu_backward(gy, saved[0], ctx.activation, ctx.bits, want, both[:, :width], both[:, width:])
                return both.view(ctx.input_shape).to(ctx.input_dtype), None, None, None, None
            d_gate, d_up = cabi_x.glu_backward(gy, saved[0], ctx.activation, ctx.bits, want)
            return (None if d_gate is None else d_gate.view(ctx.shape).to(ctx.input_dtype), None if d_up is None else d_up.view(ctx.shape).to(ctx.up_dtype),
                    None, None, None)


def glu_quantized(gate: torch.Tensor, up: Optional[torch.Tensor] = None, activation: str = 'silu', bits: int = 4,
                  generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """``act(gate) * up`` that keeps ``gate`` and ``up`` in ``bits`` = 2, 4 or 8 bits per element each, rounded without bias, instead of ``gate``,
    ``act(gate)`` and ``up``: the output is the exact product (``act`` in fp32, one product, rounded once), both gradients carry a bias of second
    order in the rounding step (module docstring).  ``up=None``: ``gate`` is ``[gate | up]`` along its last dimension (the output of ONE fused
    projection), and its one gradient tensor is written by the one backward launch without a copy.  Two tensors may be any views with unit last
    stride and one row stride (``x.chunk(2, -1)``); other layouts are gathered first.  ``activation``: ``'silu'`` or ``'gelu'`` (the erf form).
    ``generator``: the source of the rounding's randomness; without it the host default generator seeds every call.  Grad mode off, or nothing
    that requires grad: the plain forward -- no seed is drawn and nothing is kept.  Inside ``torch.utils.checkpoint`` ``generator`` must be a
    default one (``None`` included)."""
    _check(activation, bits)
    if up is not None and up.shape != gate.shape:
        raise ValueError(f'up should have the shape of gate, {tuple(gate.shape)}, but got {tuple(up.shape)}.')
    if up is None:
        _halves(gate)                                                                          # (the refusal of an odd width)
    if not kept.trains(gate, up):
        g, u = _halves(gate.detach()) if up is None else (gate.detach(), up.detach())
        if not _kernel_applies(g, u):
            return _torch_product(g, u, activation)
        return cabi_x.glu_forward(_rows(g), _rows(u), activation, keep=False)[0].view(g.shape)
    return _GLUQuantized.apply(gate, up, activation, int(bits), generator)


class _GatedMLPQuantized(torch.autograd.Function):
    """``down(act(gate(x)) * up(x))`` as ONE node (:func:`gated_mlp_quantized`).  Kept for backward on the kernels: the packed form of ``x`` (one
    uint8 buffer, ``cabi_x.quant_pack``; only while ``gate_weight`` or ``up_weight`` requires grad), the state of gate and up (one uint8 buffer,
    ``cabi_x.glu_forward``; only while something other than ``down_bias`` requires grad) and the three weights; in the PyTorch formulation the
    codes (one per byte), lo and step of every group of each.  On ``ctx``: the two seeds (ints; device words while the stream is being captured;
    None where nothing is rounded) and ``layout``, how many of the saved tensors are those of ``x`` and those of gate and up (the three weights follow).
    Nothing of the shape of ``x``, ``gate``, ``up`` or ``y`` in a float dtype."""

    @staticmethod
    def forward(ctx, x, gate_weight, up_weight, down_weight, gate_bias, up_bias, down_bias, activation: str, bits: int, generator):
        needs = ctx.needs_input_grad
        ctx.activation, ctx.bits, ctx.input_shape, ctx.input_dtype = activation, bits, tuple(x.shape), x.dtype
        ctx.autocast = linear._autocast_seen(x.device.type)
        keeps_x, keeps_gate_up = needs[1] or needs[2], any(needs[:6])
        flat = x.detach().reshape(-1, x.shape[-1])
        gate, up = F.linear(x, gate_weight, gate_bias), F.linear(x, up_weight, up_bias)
        lead, width = gate.shape[:-1], gate.shape[-1]
        gate, up = gate.reshape(-1, width), up.reshape(-1, width)
        ctx.flat_shape, ctx.width = tuple(flat.shape), width
        native = _kernel_applies(gate, up) and flat.dtype in DTYPES
        # two seeds wherever the kernels round anything (also where x^ is not kept: the stream of the generator does not depend on what is frozen), seed_x
        # first, both before anything is packed.  ONE would not do: the packed form and the gate part of the state both round in counter domain 7, so x^
        # and g^ would meet the same uniforms at the same flat indices and E[d_gate^T x^] would no longer factor.  Only down_bias is trained: its
        # gradient is a column sum of the incoming one, nothing is rounded, no seed is drawn
        ctx.seeds = (linear._sketch_seed(generator, flat.device), linear._sketch_seed(generator, flat.device)) if native and keeps_gate_up else None
        x_kept = kept.keep(flat, bits, ctx.seeds[0] if native else None, generator) if keeps_x else ()
        if native:
            y, state = cabi_x.glu_forward(gate, up, activation, bits, ctx.seeds[1] if keeps_gate_up else 0, keeps_gate_up)
            gate_up_kept = (state, ) if keeps_gate_up else ()
        else:
            gate_up_kept = kept.quantize_groups(gate, bits, generator) + kept.quantize_groups(up, bits, generator) if keeps_gate_up else ()
            y = _torch_product(gate, up, activation)
        ctx.layout = (len(x_kept), len(gate_up_kept))           # how many of the saved tensors are x^, and gate and up; the three weights follow
        ctx.save_for_backward(*x_kept, *gate_up_kept, gate_weight, up_weight, down_weight)
        return F.linear(y.view(*lead, width), down_weight, down_bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        with linear._autocast_as(ctx.autocast):
            return _GatedMLPQuantized._backward(ctx, linear._dense_rows(grad_output))

    @staticmethod
    def _backward(ctx, grad_output):
        saved = ctx.saved_tensors                           # read once: a non-re-entrant checkpoint unpacks a saved tensor one time only
        of_x, of_gate_up = ctx.layout
        x_kept, gate_up_kept, (gate_weight, up_weight, down_weight) = saved[:of_x], saved[of_x:of_x + of_gate_up], saved[of_x + of_gate_up:]
        needs = ctx.needs_input_grad
        rows, width = ctx.flat_shape[0], ctx.width
        native = ctx.seeds is not None
        G = grad_output.reshape(-1, grad_output.shape[-1])
        if native and G.dtype not in DTYPES:
            G = G.float()
        want = (needs[0] or needs[1] or needs[4], needs[0] or needs[2] or needs[5], needs[3])       # d_gate, d_up, the product
        d_y = G @ down_weight if want[0] or want[1] else None
        d_gate = d_up = product = None
        if native and any(want):
            if d_y is not None and d_y.dtype not in DTYPES:
                d_y = d_y.float()
            dtype = G.dtype if d_y is None else d_y.dtype
            if want[0] and want[1]:
                # [d_gate | d_up] in ONE buffer: the launch writes its two halves where they lie (row stride 2 width)
                both = torch.empty((rows, 2 * width), dtype=dtype, device=G.device)
                d_gate, d_up = both[:, :width], both[:, width:]
            elif want[0] or want[1]:
                d_gate = torch.empty((rows, width), dtype=dtype, device=G.device) if want[0] else None
                d_up = torch.empty((rows, width), dtype=dtype, device=G.device) if want[1] else None
            # (y^ in the gradient's dtype, 8-bit bf16 included: the tensor it stands for, y in bf16, is itself rounded to that grid)
            product = torch.empty((rows, width), dtype=dtype, device=G.device) if want[2] else None
            cabi_x.glu_backward_product(d_y, gate_up_kept[0], ctx.activation, ctx.bits, want, d_gate, d_up, product)
        elif any(want):
            d_gate, d_up, product = _formula_backward(d_y, gate_up_kept[:3], gate_up_kept[3:], (rows, width), ctx.activation, want)
            d_gate, d_up = (None if d is None else d.to(d_y.dtype) for d in (d_gate, d_up))
            product = None if product is None else product.to(G.dtype)
        grads = [None] * 10
        if needs[3]:
            grads[3] = (G.T @ product).to(down_weight.dtype)
        if needs[6]:
            grads[6] = G.sum(dim=0)
        if needs[1] or needs[2]:
            # x^ decoded ONCE for both products, in the gradient's dtype (a bf16 gradient at 8 bits: in fp32, two terms, as in QuantizedLinear)
            by_gate, by_up = kept.products((d_gate if needs[1] else None, d_up if needs[2] else None), x_kept, ctx.flat_shape, ctx.bits)
            if needs[1]:
                grads[1] = by_gate.to(gate_weight.dtype)
            if needs[2]:
                grads[2] = by_up.to(up_weight.dtype)
        if needs[4]:
            grads[4] = d_gate.sum(dim=0)
        if needs[5]:
            grads[5] = d_up.sum(dim=0)
        if needs[0]:
            # (two products into one sum: the weights are never concatenated)
            dx = torch.addmm(d_gate @ gate_weight, d_up, up_weight)
            grads[0] = dx.view(ctx.input_shape).to(ctx.input_dtype)
        return tuple(grads)


def _plain_gated_mlp(x, gate_weight, up_weight, down_weight, gate_bias, up_bias, down_bias, activation: str) -> torch.Tensor:
    """the forward that keeps nothing (no gradient can follow): on the kernel path the product with the bytes of the keeping call"""
    gate, up = F.linear(x, gate_weight, gate_bias), F.linear(x, up_weight, up_bias)
    if _kernel_applies(gate, up) and x.dtype in DTYPES:
        width = gate.shape[-1]
        y = cabi_x.glu_forward(gate.reshape(-1, width), up.reshape(-1, width), activation, keep=False)[0].view(gate.shape)
    else:
        y = _torch_product(gate, up, activation)
    return F.linear(y, down_weight, down_bias)


def gated_mlp_quantized(x: torch.Tensor, gate_weight: torch.Tensor, up_weight: torch.Tensor, down_weight: torch.Tensor,
                        gate_bias: Optional[torch.Tensor] = None, up_bias: Optional[torch.Tensor] = None, down_bias: Optional[torch.Tensor] = None,
                        activation: str = 'silu', bits: int = 4, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """``F.linear(act(F.linear(x, gate_weight, gate_bias)) * F.linear(x, up_weight, up_bias), down_weight, down_bias)``, the gated MLP of the Llama
    family, as ONE node that keeps ``x`` in the packed form of a seed (``bits`` = 2, 4 or 8 bits per element, as :func:`linear_quantized` keeps
    it), ``gate`` and ``up`` in the state of :func:`glu_quantized`, and NOTHING of the product ``y``: three plain ``nn.Linear`` layers around
    ``glu_quantized`` keep ``x`` and ``y`` in full, and ``y`` is the widest tensor of the block.  Per token of H = 4096, I = 11008 in bf16 at 4
    bits: 2560 + 13760 bytes instead of 8192 + 13760 + 22016.

    * The forward is the three GEMMs of torch and the product kernel: the output has the bytes of the unfused composition.
    * Backward: ``d_y = G @ down_weight``; ONE launch (``cabi_x.glu_backward_product``) writes ``d_gate``, ``d_up`` and rebuilds
      ``y^ = act(g^) * u^``, the forward's own expression on the decodes; ``d down_weight = G^T y^``, ``d gate_weight = d_gate^T x^``,
      ``d up_weight = d_up^T x^`` with ``x^`` decoded once, ``dx = d_gate @ gate_weight + d_up @ up_weight``; the bias gradients are column sums.
    * ``d_gate`` and ``d_up`` carry the bias of second order in the step that :func:`glu_quantized` states, and so does ``d down_weight``: the
      two roundings are independent, so ``E[y^] = E[act(g^)] * u``, and ``act`` is not linear (tests/test_gated_mlp_host.py checks the mean of many
      seeds against the exact expectation).  ``E[x^] = x``, rounded with a seed of its own, independent of ``g^`` and ``u^``.
    * ``y^`` is written in the gradient's dtype, a bf16 gradient at 8 bits included: unlike ``X^`` of ``QuantizedLinear``, the exact tensor it
      stands for (``y`` in bf16) is itself rounded to that grid, and torch's own ``d down_weight`` carries that rounding.  ``x^`` of a bf16
      gradient at 8 bits is decoded in two terms, as in ``QuantizedLinear``.
    * Seeds: TWO per call from ``linear._sketch_seed``, the one of ``x`` first: a call moves the host generator by two draws, or by none where only
      ``down_bias`` requires grad and nothing is rounded (one seed would round ``x^`` and ``g^`` with the same uniforms at equal flat indices:
      both round in counter domain 7).  While the stream is being captured into a hipGraph they are two device words (one eager call on the
      device precedes a capture).
    * Only what a requested gradient can need is kept: the packed ``x`` only while ``gate_weight`` or ``up_weight`` requires grad.  Grad mode
      off, or nothing that requires grad: the plain forward -- no seed is drawn, nothing is kept, the same bytes.
    * The kernels serve fp32 / fp16 / bf16 GPU tensors while ``linear.use_native_sketch()`` is on; host tensors, float64 and
      ``use_native_sketch(False)`` take the PyTorch formulation of the same definition (``kept.quantize_groups``).
    * Backward runs under the autocast state the forward saw; not differentiable twice; inside ``torch.utils.checkpoint`` ``generator`` must be
      a default one (``None`` included)."""
    _check(activation, bits)
    tensors = (x, gate_weight, up_weight, down_weight, gate_bias, up_bias, down_bias)
    if not kept.trains(*tensors) or x.numel() == 0:
        if x.numel() == 0:
            return F.linear(_torch_product(F.linear(x, gate_weight, gate_bias), F.linear(x, up_weight, up_bias), activation), down_weight, down_bias)
        return _plain_gated_mlp(*(None if t is None else t.detach() for t in tensors), activation)
    return _GatedMLPQuantized.apply(*tensors, activation, int(bits), generator)


class QuantizedGLU(torch.nn.Module):
    r"""``act(gate) * up`` of a gated MLP that keeps both inputs in ``bits`` bits per element for backward (:func:`glu_quantized`).

    Parameters
    ----------
    activation : {'silu', 'gelu'}, default='silu'
        ``gelu`` is the erf form.
    bits : {2, 4, 8}, default=4
        Bits per kept element.  Groups of 64 elements share a minimum and a step (8 more bytes per group): two bf16 inputs are kept in 0.1875,
        0.3125 or 0.5625 of their bytes, where torch keeps them and ``act(gate)`` in full.
    generator : torch.Generator, optional
        Source of the rounding's randomness; without it the host default generator seeds every call (inside ``torch.utils.checkpoint``: a
        default generator).

    ``forward(gate, up)``, or ``forward(packed)`` with ``packed = [gate | up]`` along the last dimension.  ``m.eval()`` keeps no state and draws no
    seed: without gradients the call is the plain forward, and gradients asked for in eval mode are those of torch's ``act(gate) * up``.

        >>> glu = fewbit.QuantizedGLU('silu', bits=4)
        >>> hidden = down_proj(glu(gate_proj(x), up_proj(x)))
    """

    def __init__(self, activation: str = 'silu', bits: int = 4, generator: Optional[torch.Generator] = None) -> None:
        _check(activation, bits)
        super().__init__()
        self.activation, self.bits, self.generator = activation, bits, generator

    def forward(self, gate: torch.Tensor, up: Optional[torch.Tensor] = None) -> torch.Tensor:
        if kept.exact_in_eval(self, gate, up):
            return _torch_product(*(_halves(gate) if up is None else (gate, up)), self.activation)
        return glu_quantized(gate, up, self.activation, self.bits, self.generator)

    def extra_repr(self) -> str:
        return f'activation={self.activation!r}, bits={self.bits}'


def _activation_of(act_fn) -> str:
    """the name of what a model calls ``act_fn``: ``nn.SiLU``, ``nn.GELU`` of the erf form, ``F.silu`` or ``F.gelu``"""
    if isinstance(act_fn, torch.nn.SiLU) or act_fn is F.silu:
        return 'silu'
    if (isinstance(act_fn, torch.nn.GELU) and act_fn.approximate == 'none') or act_fn is F.gelu:
        return 'gelu'
    raise ValueError(f'the activation of a gated MLP should be nn.SiLU, nn.GELU(approximate=\'none\'), F.silu or F.gelu, but got {act_fn!r}.')


class QuantizedGatedMLP(torch.nn.Module):
    r"""``down_proj(act(gate_proj(x)) * up_proj(x))``, the MLP of the Llama / Mistral / Qwen / Gemma / T5-v1.1 family, whose product keeps its two
    inputs in ``bits`` bits per element (:class:`QuantizedGLU`).  The projections are plain ``nn.Linear`` layers named as in those models.

    Parameters: ``in_features``, ``hidden_features`` (the intermediate width), ``bias`` (default False), ``activation`` (``'silu'`` or ``'gelu'``),
    ``bits``, ``generator``, ``device``, ``dtype``, and ``fused`` (default False): the whole MLP as ONE node (:func:`gated_mlp_quantized`) that
    keeps ``x`` in ``bits`` bits as well and nothing of the product, where the default keeps ``x`` and the product in full for the three ``nn.Linear``
    layers.  In ``eval()`` mode gradients that are asked for are torch's exact ones either way.

        >>> swap = lambda m, path: fewbit.QuantizedGatedMLP.from_mlp(m, bits=4) if type(m).__name__.endswith('MLP') else m
        >>> model = fewbit.map_module(model, swap)
    """

    def __init__(self, in_features: int, hidden_features: int, bias: bool = False, activation: str = 'silu', bits: int = 4,
                 generator: Optional[torch.Generator] = None, device=None, dtype=None, fused: bool = False) -> None:
        super().__init__()
        self.fused = bool(fused)
        self.gate_proj = torch.nn.Linear(in_features, hidden_features, bias, device, dtype)
        self.up_proj = torch.nn.Linear(in_features, hidden_features, bias, device, dtype)
        self.down_proj = torch.nn.Linear(hidden_features, in_features, bias, device, dtype)
        self.glu = QuantizedGLU(activation, bits, generator)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self.fused:
            return self.down_proj(self.glu(self.gate_proj(x), self.up_proj(x)))
        gate, up, down, glu = self.gate_proj, self.up_proj, self.down_proj, self.glu
        if kept.exact_in_eval(self, x, *self.parameters()):
            return down(_torch_product(gate(x), up(x), glu.activation))
        return gated_mlp_quantized(x, gate.weight, up.weight, down.weight, gate.bias, up.bias, down.bias, glu.activation, glu.bits, glu.generator)

    def extra_repr(self) -> str:
        return f'fused={self.fused}'

    @classmethod
    def from_mlp(cls, module: torch.nn.Module, bits: int = 4, generator: Optional[torch.Generator] = None, fused: bool = False) -> 'QuantizedGatedMLP':
        """A ``QuantizedGatedMLP`` that SHARES the three projections of ``module``: any module with ``gate_proj``, ``up_proj``, ``down_proj`` and an
        ``act_fn`` that is ``nn.SiLU``, ``nn.GELU()`` of the erf form, ``F.silu`` or ``F.gelu`` (``LlamaMLP`` and its kin), so that ``map_module``
        can swap the MLPs of a built model.  Any other ``act_fn``: ``ValueError``."""
        missing = [name for name in ('gate_proj', 'up_proj', 'down_proj', 'act_fn') if not hasattr(module, name)]
        if missing:
            raise TypeError(f'{type(module).__name__} has no {", ".join(missing)}: not a gated MLP of the gate_proj / up_proj / down_proj kind')
        activation = _activation_of(module.act_fn)
        new = cls(1, 1, activation=activation, bits=bits, generator=generator, device='meta', fused=fused)
        new.gate_proj, new.up_proj, new.down_proj = module.gate_proj, module.up_proj, module.down_proj
        return new.train(module.training)
