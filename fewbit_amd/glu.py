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
  ``linear._quantize_groups``, backward is the formula above.
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

from . import cabi_x, linear
from .cabi import DTYPES

__all__ = ('glu_quantized', 'QuantizedGLU', 'QuantizedGatedMLP')

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
    return (linear.use_native_sketch() and gate.device.type == 'cuda' and gate.dtype in DTYPES and up.dtype == gate.dtype and up.device == gate.device
            and 0 < gate.numel() <= 2**36)


def _slope(g: torch.Tensor, activation: str) -> torch.Tensor:
    """``act'`` of the definition: silu ``s (1 + g (1 - s))``, gelu ``Phi(g) + g phi(g)``"""
    if activation == 'silu':
        s = torch.sigmoid(g)
        return s * (1 + g * (1 - s))
    return 0.5 * (1 + torch.erf(g * math.sqrt(0.5))) + g * torch.exp(-0.5 * g * g) * (1 / math.sqrt(2 * math.pi))


def _decoded(codes: torch.Tensor, lo: torch.Tensor, step: torch.Tensor, shape) -> torch.Tensor:
    values = torch.addcmul(lo[:, None], codes.view(-1, cabi_x.QUANT_GROUP).to(lo.dtype), step[:, None])
    return values.reshape(-1)[:math.prod(shape)].view(shape)


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
        ctx.save_for_backward(*linear._quantize_groups(g, bits, generator), *linear._quantize_groups(u, bits, generator))
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
                work = saved[1].dtype
                g, u = _decoded(*saved[:3], ctx.shape), _decoded(*saved[3:], ctx.shape)
                poisoned = torch.isnan(g) | torch.isnan(u)
                gy = grad_output.to(work)
                nan = torch.full((), float('nan'), dtype=work, device=gy.device)
                d_up = torch.where(poisoned, nan, gy * (F.silu(g) if ctx.activation == 'silu' else F.gelu(g))) if want[1] else None
                d_gate = torch.where(poisoned, nan, gy * u * _slope(g, ctx.activation)) if want[0] else None
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
    if bits not in cabi_x.QUANT_BITS:
        raise ValueError(f'bits should be 2, 4 or 8, but got {bits}.')
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation should be 'silu' or 'gelu', but got {activation!r}.")
    if up is not None and up.shape != gate.shape:
        raise ValueError(f'up should have the shape of gate, {tuple(gate.shape)}, but got {tuple(up.shape)}.')
    if up is None:
        _halves(gate)                                                                          # (the refusal of an odd width)
    if not torch.is_grad_enabled() or not any(t is not None and t.requires_grad for t in (gate, up)):
        g, u = _halves(gate.detach()) if up is None else (gate.detach(), up.detach())
        if not _kernel_applies(g, u):
            return _torch_product(g, u, activation)
        return cabi_x.glu_forward(_rows(g), _rows(u), activation, keep=False)[0].view(g.shape)
    return _GLUQuantized.apply(gate, up, activation, int(bits), generator)


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
        if bits not in cabi_x.QUANT_BITS:
            raise ValueError(f'bits should be 2, 4 or 8, but got {bits}.')
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation should be 'silu' or 'gelu', but got {activation!r}.")
        super().__init__()
        self.activation, self.bits, self.generator = activation, bits, generator

    def forward(self, gate: torch.Tensor, up: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not self.training and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (gate, up)):
            # eval mode is not where activation memory is short: gradients asked for there are torch's exact ones, nothing is rounded or drawn
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
    ``bits``, ``generator``, ``device``, ``dtype``.

        >>> swap = lambda m, path: fewbit.QuantizedGatedMLP.from_mlp(m, bits=4) if type(m).__name__.endswith('MLP') else m
        >>> model = fewbit.map_module(model, swap)
    """

    def __init__(self, in_features: int, hidden_features: int, bias: bool = False, activation: str = 'silu', bits: int = 4,
                 generator: Optional[torch.Generator] = None, device=None, dtype=None) -> None:
        super().__init__()
        self.gate_proj = torch.nn.Linear(in_features, hidden_features, bias, device, dtype)
        self.up_proj = torch.nn.Linear(in_features, hidden_features, bias, device, dtype)
        self.down_proj = torch.nn.Linear(hidden_features, in_features, bias, device, dtype)
        self.glu = QuantizedGLU(activation, bits, generator)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.down_proj(self.glu(self.gate_proj(x), self.up_proj(x)))

    @classmethod
    def from_mlp(cls, module: torch.nn.Module, bits: int = 4, generator: Optional[torch.Generator] = None) -> 'QuantizedGatedMLP':
        """A ``QuantizedGatedMLP`` that SHARES the three projections of ``module``: any module with ``gate_proj``, ``up_proj``, ``down_proj`` and an
        ``act_fn`` that is ``nn.SiLU``, ``nn.GELU()`` of the erf form, ``F.silu`` or ``F.gelu`` (``LlamaMLP`` and its kin), so that ``map_module``
        can swap the MLPs of a built model.  Any other ``act_fn``: ``ValueError``."""
        missing = [name for name in ('gate_proj', 'up_proj', 'down_proj', 'act_fn') if not hasattr(module, name)]
        if missing:
            raise TypeError(f'{type(module).__name__} has no {", ".join(missing)}: not a gated MLP of the gate_proj / up_proj / down_proj kind')
        activation = _activation_of(module.act_fn)
        new = cls(1, 1, activation=activation, bits=bits, generator=generator, device='meta')
        new.gate_proj, new.up_proj, new.down_proj = module.gate_proj, module.up_proj, module.down_proj
        return new.train(module.training)
