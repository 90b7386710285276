"""LayerNorm and RMSNorm that keep their normalized input in 2, 4 or 8 bits per element for backward.

``torch.nn.LayerNorm`` saves its whole input plus a mean and an rstd per row, and in a transformer that input is the residual sum, which no
other node saves.  Here the node keeps the NORMALIZED rows ``x^ = (x - mean) * rstd`` in the packed form of a seed (include/fewbit_hipx.h, "the
normalized rows of a seed": per 64 elements of a row a minimum and a step, per element a code rounded stochastically and without bias) plus
one fp32 ``rstd`` per row: at 4 bits 0.3125 of a bf16 input's bytes.  ``x^`` is close to N(0, 1) in every row, the distribution a min / step
code per 64 elements suits best, and backward needs nothing else but gamma.

* The forward value is the exact layer norm; only the gradients see the rounding.  ``dgamma = sum_r gy * x^q`` is unbiased (``E[x^q] = x^``);
  ``dbeta`` is exact.  ``dx = rstd * (g^ - mean(g^) - x^q * mean(g^ * x^q))`` with ``g^ = gy * gamma`` is NOT exactly unbiased: ``x^q`` enters it
  twice, so ``E[dx_q] - dx = -rstd * g^_i * Var(x^q_i) / width``, second order in the step and divided by the width (tests/test_norm_host.py
  measures the sum of both against the noise of one call).
* The kernels (fewbit_amd/csrc/fewbit_norm.hip: one launch forward, two backward) serve fp32 / fp16 / bf16 GPU tensors with a flattened
  normalized width of 1 .. 8192 and gamma / beta of the input's dtype (or absent) while ``linear.use_native_sketch()`` is on.  Host tensors,
  float64, wider rows and ``use_native_sketch(False)`` take a PyTorch formulation of the same definition: ``y`` is ``F.layer_norm``'s, the codes
  come from ``kept.quantize_groups`` on the rows of ``x^`` padded to whole groups, backward is the formula above.
* The seed comes from ``linear._sketch_seed``: an int drawn from the host generator, or a device word while the stream is being captured into
  a hipGraph -- a captured layer draws fresh roundings on every replay and its recorded backward reads the state its forward wrote.  (One eager
  call on the device precedes a capture, as for the randomized linears.)
* With grad mode off, or when neither the input nor gamma nor beta requires grad, the call is the plain forward: no seed is drawn, no state
  is written, no node is built; on the kernel path ``y`` has the bytes of the keeping call.
* Under ``torch.autocast`` the output of the kernel path keeps the INPUT's dtype (the arithmetic inside is fp32 whatever the dtype, fp32
  parameters are cast to the input's dtype first); torch's ``layer_norm`` would return fp32 there.  Backward runs under the autocast state
  the forward saw (``linear._autocast_as``), so ``backward()`` may follow the block.
* Inside ``torch.utils.checkpoint`` the generator must be a default one (``generator=None``, ``torch.default_generator``,
  ``torch.cuda.default_generators[i]``): checkpoint saves and restores only those, and the recomputation must draw the forward's seed again.
* A row with a NaN or an infinity gives NaN in that row of ``y`` and ``dx`` and in every column of ``dgamma``, as with torch.
* Not differentiable twice (``once_differentiable``).

``QuantizedRMSNorm`` / ``rms_norm_quantized`` are the same node for ``torch.nn.RMSNorm`` (every model of the Llama / Mistral / Qwen / T5 family):
``x^ = x * rstd`` with ``rstd = 1 / sqrt(mean(x^2) + eps)``, ``y = x^ * gamma``, the same state of ``x^``, and backward without the mean term and
without beta: ``dx = rstd * (g^ - x^q * mean(g^ * x^q))``, ``dgamma = sum_r gy * x^q`` (include/fewbit_hipx.h, "The un-centred rows").  Every rule
above holds for it; the bias of ``dx`` is the same ``-rstd * g^_i * Var(x^q_i) / width``.  Its non-finite values are those of the fp32 arithmetic
and of torch's own formulation: a NaN element makes its row NaN; an INFINITE element makes ``mean(x^2)`` infinite, so ``rstd`` is 0 and ``x^`` is
NaN at that element and +-0 elsewhere -- the group that holds it is poisoned, ``dx`` of the row is NaN and ``dgamma`` is NaN in that group's
columns.  A finite row whose fp32 sum of squares overflows (bf16 values near 1e20) gives ``rstd`` = 0 and ``y`` = +-0.

``DropoutAddLayerNorm`` / ``DropoutAddRMSNorm`` (``dropout_add_layer_norm_quantized`` / ``dropout_add_rms_norm_quantized``) are a sublayer's whole
ending, ``y = norm(residual + dropout(input))``, as ONE node: one seed per call (the mask and the rounding are two Philox domains of it), one
launch forward and two backward where ``dropout_add`` followed by the quantized norm takes two and three.  Kept: the state, ``rstd``, gamma and,
on ``ctx``, the seed and ``p`` -- no mask, and not the sum ``h``, which post-norm (``prenorm=False``) is never in memory.  With ``prenorm=True``
the call returns ``(y, h)`` and the gradient arriving at ``h`` is added inside the backward kernel.  The values are the composition's, bit for bit
(include/fewbit_hipx.h, "The sum of a seed in front of the norm").  The kernel path is that of the plain norms plus a residual of the input's
shape, dtype and device plus, with a mask, a width that is a multiple of 8; everything else IS the composition of ``dropout_add`` and the
quantized norm (two seeds).  Grad mode off or nothing that requires grad: the plain fused forward, which still drops while ``training and p > 0``.
Every rule above -- autocast, checkpoint, capture, non-finite values, ``once_differentiable`` -- holds for it.
"""
import math
from typing import Optional, Sequence, Union

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import cabi_x, kept, linear
from .cabi import DTYPES
from .dropout import _check_p, dropout_add

__all__ = ('layer_norm_quantized', 'QuantizedLayerNorm', 'rms_norm_quantized', 'QuantizedRMSNorm', 'dropout_add_layer_norm_quantized', 'DropoutAddLayerNorm',
           'dropout_add_rms_norm_quantized', 'DropoutAddRMSNorm')

# Everything below takes the kind as ``centred``: True for the layer norm, False for the RMS norm (the un-centred statistic, backward without the mean
# term, no beta: ``bias`` is None throughout).


def _kernel_applies(flat: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor]) -> bool:
    if not (linear._kernels_take(flat) and 1 <= flat.shape[1] <= cabi_x.NORM_MAX_WIDTH):
        return False
    # (under autocast fp32 parameters meet a 16-bit input: they are cast to it, a copy of `width` elements)
    cast = torch.is_autocast_enabled('cuda')
    return all(p is None or (p.device == flat.device and (p.dtype == flat.dtype or (cast and p.dtype in DTYPES))) for p in (weight, bias))


def _as(p: Optional[torch.Tensor], dtype: torch.dtype) -> Optional[torch.Tensor]:
    return None if p is None else p.detach().reshape(-1).to(dtype).contiguous()


def _torch_norm(centred: bool, input, normalized_shape, weight, bias, eps):
    return F.layer_norm(input, normalized_shape, weight, bias, eps) if centred else F.rms_norm(input, normalized_shape, weight, eps)


def _kernel_forward(centred: bool, flat, weight, bias, eps, bits: int = 4, seed=0, keep: bool = True, residual=None, p: float = 0.0, want_h: bool = False):
    """(y, h, rstd, state) of the entry point of the kind on the rows of ``flat``; with a ``residual`` (2-D as well) the fused entry point, which normalizes
    ``h = residual + dropout(flat)`` and returns it with ``want_h`` (else, and without a residual, ``h`` is None)"""
    flat = flat if flat.is_contiguous() else flat.contiguous()
    parameters = (_as(weight, flat.dtype), _as(bias, flat.dtype)) if centred else (_as(weight, flat.dtype), )
    if residual is None:
        y, rstd, state, _ = (cabi_x.layer_norm_forward if centred else cabi_x.rms_norm_forward)(flat, *parameters, eps, bits, seed, keep)
        return y, None, rstd, state
    call = cabi_x.add_layer_norm_forward if centred else cabi_x.add_rms_norm_forward
    return call(flat, residual if residual.is_contiguous() else residual.contiguous(), *parameters, eps, p, bits, seed, keep, want_h)[:4]


def _row_statistic(flat: torch.Tensor, eps: float, centred: bool):
    """(x^, rstd) of the rows of ``flat`` in fp32 (fp64 for a float64 input): the two-pass variance of the definition, or, un-centred,
    ``x^ = x * rstd`` with ``rstd = 1 / sqrt(mean(x^2) + eps)``"""
    work = flat.to(torch.float64 if flat.dtype == torch.float64 else torch.float32)
    if centred:
        work = work - work.mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(work.square().mean(dim=1, keepdim=True) + eps)
    return work * rstd, rstd.reshape(-1)


def _padded_rows(xhat: torch.Tensor) -> torch.Tensor:
    """the rows filled up to whole groups with their last element, which moves neither a group's minimum nor its maximum"""
    pad = -xhat.shape[1] % cabi_x.QUANT_GROUP
    return torch.cat((xhat, xhat[:, -1:].expand(-1, pad)), dim=1) if pad else xhat


def _backward_formula(gy: torch.Tensor, xq: torch.Tensor, rstd: torch.Tensor, gamma: Optional[torch.Tensor], centred: bool):
    """(dx, dgamma, dbeta) of the definition in the dtype of ``xq``; un-centred the mean term is absent and ``dbeta`` is None"""
    gy = gy.to(xq.dtype)
    gh = gy if gamma is None else gy * gamma.reshape(1, -1).to(xq.dtype)
    deviation = gh - gh.mean(dim=1, keepdim=True) if centred else gh
    dx = rstd[:, None] * (deviation - xq * (gh * xq).mean(dim=1, keepdim=True))
    return dx, (gy * xq).sum(dim=0), gy.sum(dim=0) if centred else None


def _node_forward(ctx, centred: bool, input, weight, bias, normalized_shape, eps: float, bits: int, generator, add=None):
    """Kept for backward on the kernels: ONE uint8 buffer (the state), ``rstd`` (fp32 per row) and gamma; in the PyTorch formulation the codes (one
    per byte), lo and step of every group, ``rstd`` and gamma.  ``add``: None, or ``(residual, p, prenorm)``: the node is then
    ``norm(residual + dropout(input))`` on the fused kernels, which have no PyTorch formulation here -- the CALLER has made sure that they apply
    (``_dropout_add_norm_quantized``).  The same tensors are kept, the ONE seed of the call and ``p`` are on ``ctx``, and with ``prenorm`` the result is
    the pair ``(y, h)``."""
    residual, p, prenorm = add or (None, 0.0, False)
    width = math.prod(normalized_shape)
    flat = input.detach().reshape(-1, width)
    ctx.bits, ctx.flat_shape, ctx.input_dtype, ctx.p = bits, tuple(flat.shape), input.dtype, p
    ctx.has_weight, ctx.normalized_shape, ctx.bias_dtype = weight is not None, tuple(normalized_shape), None if bias is None else bias.dtype
    ctx.autocast = linear._autocast_seen(input.device.type)
    ctx.native_seed = None
    if add is not None or _kernel_applies(flat, weight, bias):
        ctx.native_seed = linear._sketch_seed(generator, flat.device)
        y, h, rstd, state = _kernel_forward(centred, flat, weight, bias, eps, bits, ctx.native_seed, True,
                                            None if add is None else residual.detach().reshape(-1, width), p, prenorm)
        ctx.save_for_backward(state, rstd, *((weight, ) if ctx.has_weight else ()))
        return (y.view(input.shape), h.view(input.shape)) if prenorm else y.view(input.shape)
    xhat, rstd = _row_statistic(flat, eps, centred)
    ctx.save_for_backward(*kept.quantize_groups(_padded_rows(xhat), bits, generator), rstd, *((weight, ) if ctx.has_weight else ()))
    return _torch_norm(centred, input, normalized_shape, weight, bias, eps)


def _node_backward(ctx, centred: bool, grad_output, fused: bool = False, grad_h=None):
    """(grad_input, grad_weight, grad_bias, grad_residual) as ``ctx.needs_input_grad`` wants them, under the autocast state the forward saw.  The inputs
    of the plain nodes are (input, weight[, bias]); ``fused``: (input, residual, weight, bias), ``grad_h`` is the gradient arriving at ``h``, and either
    gradient may be None."""
    with linear._autocast_as(ctx.autocast):
        saved = ctx.saved_tensors                       # read once: a non-re-entrant checkpoint unpacks a saved tensor one time only
        weight = saved[-1] if ctx.has_weight else None
        rows, width = ctx.flat_shape
        needs = ctx.needs_input_grad
        if fused:
            want_input, want_residual, want_weight, want_bias = needs[:4]
            shape = (grad_output if grad_output is not None else grad_h).shape
            if grad_output is None:                     # (only h reached the loss: the norm's own terms are those of a zero gradient)
                grad_output = torch.zeros_like(grad_h)
        else:
            want_input, want_weight, want_bias, want_residual, shape = needs[0], needs[1], centred and needs[2], False, grad_output.shape
        gy = linear._dense_rows(grad_output).reshape(rows, width)
        sums = (want_weight, want_bias) if centred else (want_weight, )
        dres = None
        if ctx.native_seed is None:
            codes, lo, step, rstd = saved[:4]
            dx, dgamma, dbeta = _backward_formula(gy, kept.decode(codes, lo, step, rows, width), rstd, weight, centred)
        elif fused:
            gy = gy if gy.dtype in DTYPES else gy.float()
            gh = None if grad_h is None else linear._dense_rows(grad_h.to(gy.dtype)).reshape(rows, width)
            mask = cabi_x.dropout_threshold(ctx.p) > 0
            # without a mask the two gradients are the same values: ONE tensor is written and returned for both
            call = cabi_x.add_layer_norm_backward if centred else cabi_x.add_rms_norm_backward
            dres, dbranch, dgamma, *dbeta = call(gy, saved[0], saved[1], _as(weight, gy.dtype), ctx.bits, ctx.native_seed, ctx.p, gh,
                                                 (want_residual or (want_input and not mask), want_input and mask, *sums))
            dx, dbeta = dbranch if mask else dres, dbeta[0] if centred else None
        else:
            gy = gy if gy.dtype in DTYPES else gy.float()
            call = cabi_x.layer_norm_backward if centred else cabi_x.rms_norm_backward
            dx, dgamma, *dbeta = call(gy, saved[0], saved[1], _as(weight, gy.dtype), ctx.bits, (want_input, *sums))
            dbeta = dbeta[0] if centred else None
        grad_input = dx.to(ctx.input_dtype).view(shape) if want_input else None
        grad_residual = dres.to(ctx.input_dtype).view(shape) if want_residual else None
        grad_weight = dgamma.to(weight.dtype).view(weight.shape) if want_weight else None
        grad_bias = dbeta.to(ctx.bias_dtype).view(ctx.normalized_shape) if want_bias else None
        return grad_input, grad_weight, grad_bias, grad_residual


class _LayerNormQuantized(torch.autograd.Function):
    """``F.layer_norm`` that keeps ``x^`` in ``bits`` bits per element (module docstring; what is kept: ``_node_forward``)"""

    @staticmethod
    def forward(ctx, input, weight, bias, normalized_shape, eps: float, bits: int, generator):
        return _node_forward(ctx, True, input, weight, bias, normalized_shape, eps, bits, generator)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return (*_node_backward(ctx, True, grad_output)[:3], None, None, None, None)


class _RMSNormQuantized(torch.autograd.Function):
    """``F.rms_norm`` that keeps ``x^`` in ``bits`` bits per element (module docstring).  Kept for backward exactly what ``_LayerNormQuantized``
    keeps."""

    @staticmethod
    def forward(ctx, input, weight, normalized_shape, eps: float, bits: int, generator):
        return _node_forward(ctx, False, input, weight, None, normalized_shape, eps, bits, generator)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return (*_node_backward(ctx, False, grad_output)[:2], None, None, None, None)


def _norm_quantized(centred: bool, input, normalized_shape, weight, bias, eps, bits, generator) -> torch.Tensor:
    """the functional front of both kinds: the refusals, the plain forward when nothing is kept, the node otherwise"""
    if bits not in cabi_x.QUANT_BITS:
        kept.check_bits(bits)                                                             # (words the refusal)
    normalized_shape = (normalized_shape, ) if isinstance(normalized_shape, int) else tuple(normalized_shape)
    if tuple(input.shape[input.dim() - len(normalized_shape):]) != normalized_shape or not normalized_shape:
        return _torch_norm(centred, input, normalized_shape, weight, bias, eps)              # (torch words the refusal)
    if not centred:                                                                       # (the default F.rms_norm documents)
        eps = float(torch.finfo(input.dtype).eps if eps is None else eps)
    # (inline, not kept.trains: a norm's step at width 768 is bound by the Python around its launches)
    if not torch.is_grad_enabled() or not any(t is not None and t.requires_grad for t in (input, weight, bias)):
        flat = input.detach().reshape(-1, math.prod(normalized_shape))
        if not _kernel_applies(flat, weight, bias):
            return _torch_norm(centred, input, normalized_shape, weight, bias, eps)
        return _kernel_forward(centred, flat, weight, bias, eps, keep=False)[0].view(input.shape)
    if centred:
        return _LayerNormQuantized.apply(input, weight, bias, normalized_shape, float(eps), int(bits), generator)
    return _RMSNormQuantized.apply(input, weight, normalized_shape, eps, int(bits), generator)


class _QuantizedNorm:
    """What the two modules share, in front of ``nn.LayerNorm`` / ``nn.RMSNorm`` in their bases: the check of ``bits``, the eval-mode rule and the
    repr.  ``_centred`` is the kind."""

    def __init__(self, bits: int, generator: Optional[torch.Generator], *norm_arguments) -> None:
        kept.check_bits(bits)
        super().__init__(*norm_arguments)
        self.bits = bits
        self.generator = generator

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        bias = self.bias if self._centred else None
        if not self.training and kept.trains(input, self.weight, bias):           # (the eval-mode rule, kept.exact_in_eval, at no cost while training)
            return _torch_norm(self._centred, input, self.normalized_shape, self.weight, bias, self.eps)
        return _norm_quantized(self._centred, input, self.normalized_shape, self.weight, bias, self.eps, self.bits, self.generator)

    def extra_repr(self) -> str:
        return f'{super().extra_repr()}, bits={self.bits}'


def layer_norm_quantized(input: torch.Tensor, normalized_shape: Union[int, Sequence[int]], weight: Optional[torch.Tensor] = None,
                         bias: Optional[torch.Tensor] = None, eps: float = 1e-5, bits: int = 4, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """``F.layer_norm(input, normalized_shape, weight, bias, eps)`` that keeps the normalized rows in ``bits`` = 2, 4 or 8 bits per element
    (plus one fp32 ``rstd`` per row) instead of the input: the output is the exact layer norm, ``grad_bias`` is exact, ``grad_weight`` is
    unbiased, ``grad_input`` carries a bias of second order in the rounding step (module docstring).  ``generator``: the source of the
    rounding's randomness; without it the host default generator seeds every call.  Grad mode off, or nothing that requires grad: the plain
    forward -- no seed is drawn and nothing is kept.  Under ``torch.autocast`` the kernel path returns the INPUT's dtype where torch returns
    fp32.  Inside ``torch.utils.checkpoint`` ``generator`` must be a default one (``None`` included): checkpoint restores only those, and the
    recomputation must draw the forward's seed again (module docstring)."""
    return _norm_quantized(True, input, normalized_shape, weight, bias, eps, bits, generator)


class QuantizedLayerNorm(_QuantizedNorm, torch.nn.LayerNorm):
    r"""Drop-in :class:`torch.nn.LayerNorm` that keeps its normalized input in ``bits`` bits per element, plus one fp32 per row, instead of the
    input itself (:func:`layer_norm_quantized`); the output is that of ``nn.LayerNorm``.

    Parameters (after those of ``nn.LayerNorm``)
    ----------
    bits : {2, 4, 8}, default=4
        Bits per kept element.  Groups of 64 elements of a row share a minimum and a step (8 more bytes per group): a bf16 input is kept in
        0.1875, 0.3125 or 0.5625 of its bytes.  The rounding is stochastic; the weight gradient is unbiased, the input gradient up to a term of
        second order in the step.
    generator : torch.Generator, optional
        Source of the rounding's randomness; without it the host default generator seeds every call.  Inside ``torch.utils.checkpoint`` the
        generator must be a default one (``None``, ``torch.default_generator``, ``torch.cuda.default_generators[i]``): checkpoint saves and
        restores only those, so a generator of the caller's own draws a second seed in the recomputation and the gradients no longer belong to
        the rounding of the forward.

    Under ``torch.autocast`` the output keeps the input's dtype on the kernel path (``nn.LayerNorm`` returns fp32 there).  ``m.eval()`` keeps no
    state and draws no seed: without gradients the call is the plain forward (the same output bytes as in training), and gradients asked for
    in eval mode are ``F.layer_norm``'s exact ones.

    Examples:

        >>> m = fewbit.QuantizedLayerNorm(768, bits=4)
        >>> model = fewbit.map_module(model, lambda m, path: fewbit.QuantizedLayerNorm.from_layer_norm(m, bits=4) if type(m) is torch.nn.LayerNorm else m)
    """

    _centred = True

    def __init__(self, normalized_shape, eps: float = 1e-5, elementwise_affine: bool = True, bias: bool = True, device=None, dtype=None, bits: int = 4,
                 generator: Optional[torch.Generator] = None) -> None:
        super().__init__(bits, generator, normalized_shape, eps, elementwise_affine, bias, device, dtype)

    @classmethod
    def from_layer_norm(cls, module: torch.nn.LayerNorm, bits: int = 4, generator: Optional[torch.Generator] = None) -> 'QuantizedLayerNorm':
        """A ``QuantizedLayerNorm`` that SHARES the parameters of ``module`` (what ``map_module`` needs to swap the norms of a built model)"""
        new = cls(module.normalized_shape, module.eps, module.elementwise_affine, module.bias is not None, device='meta', bits=bits, generator=generator)
        new.weight, new.bias = module.weight, module.bias
        return new.train(module.training)



def rms_norm_quantized(input: torch.Tensor, normalized_shape: Union[int, Sequence[int]], weight: Optional[torch.Tensor] = None, eps: Optional[float] = None,
                       bits: int = 4, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """``F.rms_norm(input, normalized_shape, weight, eps)`` that keeps the normalized rows ``x * rstd`` in ``bits`` = 2, 4 or 8 bits per element
    (plus one fp32 ``rstd`` per row) instead of the input: the output is the exact RMS norm (``x^ * gamma`` in fp32, rounded ONCE), ``grad_weight``
    is unbiased, ``grad_input`` carries the bias ``-rstd * g^_i * Var(x^q_i) / width``, second order in the rounding step (module docstring).
    ``eps=None`` means ``torch.finfo(input.dtype).eps``, the default ``F.rms_norm`` documents (for a 16-bit host tensor torch 2.10's own
    composite takes the epsilon of its fp32 arithmetic instead; pass ``eps`` to be independent of that).  ``generator``, grad mode off, ``torch.autocast`` and
    ``torch.utils.checkpoint``: the rules of :func:`layer_norm_quantized`."""
    return _norm_quantized(False, input, normalized_shape, weight, None, eps, bits, generator)


class QuantizedRMSNorm(_QuantizedNorm, torch.nn.RMSNorm):
    r"""Drop-in :class:`torch.nn.RMSNorm` that keeps its normalized input in ``bits`` bits per element, plus one fp32 per row, instead of the
    input itself (:func:`rms_norm_quantized`); the output is that of ``nn.RMSNorm``.

    Parameters (after those of ``nn.RMSNorm``)
    ----------
    bits : {2, 4, 8}, default=4
        Bits per kept element.  Groups of 64 elements of a row share a minimum and a step (8 more bytes per group): a bf16 input is kept in
        0.1875, 0.3125 or 0.5625 of its bytes.  The rounding is stochastic; the weight gradient is unbiased, the input gradient up to
        ``-rstd * g^_i * Var(x^q_i) / width``, a term of second order in the step.
    generator : torch.Generator, optional
        Source of the rounding's randomness, as for :class:`QuantizedLayerNorm` (inside ``torch.utils.checkpoint``: a default generator).

    Under ``torch.autocast`` the output keeps the input's dtype on the kernel path.  ``m.eval()`` keeps no state and draws no seed: without
    gradients the call is the plain forward, and gradients asked for in eval mode are ``F.rms_norm``'s exact ones.

    Examples:

        >>> m = fewbit.QuantizedRMSNorm(4096, eps=1e-6, bits=4)
        >>> swap = lambda m, path: fewbit.QuantizedRMSNorm.from_rms_norm(m, bits=4) if type(m).__name__.endswith('RMSNorm') else m
        >>> model = fewbit.map_module(model, swap)
    """

    _centred = False

    def __init__(self, normalized_shape, eps: Optional[float] = None, elementwise_affine: bool = True, device=None, dtype=None, bits: int = 4,
                 generator: Optional[torch.Generator] = None) -> None:
        super().__init__(bits, generator, normalized_shape, eps, elementwise_affine, device, dtype)

    @classmethod
    def from_rms_norm(cls, module: torch.nn.Module, bits: int = 4, generator: Optional[torch.Generator] = None) -> 'QuantizedRMSNorm':
        """A ``QuantizedRMSNorm`` that SHARES the weight of ``module``: a ``torch.nn.RMSNorm``, or any module with a 1-D ``weight`` and a float
        ``variance_epsilon`` or ``eps`` (the ``LlamaRMSNorm`` / ``T5LayerNorm`` family of Hugging Face models), so that ``map_module`` can swap
        the norms of a built model.  Those modules round ``x^`` to the input's dtype BEFORE they multiply by the weight; here ``x^ * weight`` is
        formed in fp32 and rounded once, so a 16-bit output may differ from theirs in its last bit."""
        if isinstance(module, torch.nn.RMSNorm):
            shape, eps, affine = module.normalized_shape, module.eps, module.elementwise_affine
        else:
            weight = getattr(module, 'weight', None)
            eps = getattr(module, 'variance_epsilon', getattr(module, 'eps', None))
            if not isinstance(weight, torch.Tensor) or weight.dim() != 1 or not isinstance(eps, float):
                raise TypeError(f'{type(module).__name__} is neither a torch.nn.RMSNorm nor a module with a 1-D weight and a float variance_epsilon or eps')
            shape, affine = tuple(weight.shape), True
        new = cls(shape, eps, affine, device='meta', bits=bits, generator=generator)
        new.weight = module.weight
        return new.train(module.training)


# ---- residual + dropout(input) fused in front of either norm (module docstring, last paragraph) ------------------------------------------------
class _DropoutAddNormQuantized(torch.autograd.Function):
    """``norm(residual + dropout(input))`` on the fused kernels, both kinds (``centred``): the plain node with a residual (``_node_forward``).  With
    ``prenorm`` the outputs are ``(y, h)`` and backward takes the gradient arriving at ``h``."""

    @staticmethod
    def forward(ctx, input, residual, weight, bias, centred: bool, normalized_shape, eps: float, bits: int, p: float, prenorm: bool, generator):
        ctx.centred = centred
        ctx.set_materialize_grads(False)
        return _node_forward(ctx, centred, input, weight, bias, normalized_shape, eps, bits, generator, (residual, p, prenorm))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output, grad_h=None):
        grad_input, grad_weight, grad_bias, grad_residual = _node_backward(ctx, ctx.centred, grad_output, True, grad_h)
        return grad_input, grad_residual, grad_weight, grad_bias, None, None, None, None, None, None, None


def _dropout_add_norm_quantized(centred: bool, input, residual, normalized_shape, weight, bias, eps, p, training, bits, prenorm, generator):
    """the functional front of both fused kinds: the refusals, the composition off the kernel path, the plain fused forward when nothing is kept, the
    node otherwise"""
    if bits not in cabi_x.QUANT_BITS:
        kept.check_bits(bits)
    _check_p(p)
    if tuple(residual.shape) != tuple(input.shape):
        raise ValueError(f'residual should have the shape of input, {tuple(input.shape)}, but got {tuple(residual.shape)}.')
    normalized_shape = (normalized_shape, ) if isinstance(normalized_shape, int) else tuple(normalized_shape)
    p = float(p) if training else 0.0
    fits = bool(normalized_shape) and tuple(input.shape[input.dim() - len(normalized_shape):]) == normalized_shape
    flat = input.detach().reshape(-1, math.prod(normalized_shape)) if fits else None
    if (not fits or not _kernel_applies(flat, weight, bias) or residual.dtype != input.dtype or residual.device != input.device
            or (cabi_x.dropout_threshold(p) > 0 and flat.shape[1] % 8 != 0)):
        h = dropout_add(input, residual, p, training, generator)
        y = _norm_quantized(centred, h, normalized_shape, weight, bias, eps, bits, generator)
        return (y, h) if prenorm else y
    if not centred:
        eps = float(torch.finfo(input.dtype).eps if eps is None else eps)
    if not torch.is_grad_enabled() or not any(t is not None and t.requires_grad for t in (input, residual, weight, bias)):
        seed = linear._sketch_seed(generator, flat.device) if cabi_x.dropout_threshold(p) > 0 else 0
        y, h, *_ = _kernel_forward(centred, flat, weight, bias, eps, seed=seed, keep=False, residual=residual.detach().reshape(flat.shape), p=p, want_h=prenorm)
        return (y.view(input.shape), h.view(input.shape)) if prenorm else y.view(input.shape)
    return _DropoutAddNormQuantized.apply(input, residual, weight, bias, centred, normalized_shape, float(eps), int(bits), p, bool(prenorm), generator)


def dropout_add_layer_norm_quantized(input: torch.Tensor, residual: torch.Tensor, normalized_shape: Union[int, Sequence[int]],
                                     weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, eps: float = 1e-5, p: float = 0.0,
                                     training: bool = True, bits: int = 4, prenorm: bool = False, generator: Optional[torch.Generator] = None):
    """``layer_norm_quantized(dropout_add(input, residual, p, training), normalized_shape, weight, bias, eps, bits)`` as ONE node with ONE seed: one
    launch forward, two backward; what is kept is the quantized norm's (the state, ``rstd``, gamma) plus the seed -- no mask and not the sum.
    Returns ``y``, or ``(y, h)`` with ``prenorm=True``, where ``h = residual + dropout(input)`` is the residual stream that goes on; the gradient
    arriving at ``h`` is added inside the backward kernel.  The values are those of the composition bit for bit, and off the kernel path (host
    tensors, a residual of another dtype, a mask at a width that is no multiple of 8, ...) the call IS that composition.  ``generator``, grad
    mode off, ``torch.autocast``, ``torch.utils.checkpoint`` and capture: the rules of :func:`layer_norm_quantized` (module docstring)."""
    return _dropout_add_norm_quantized(True, input, residual, normalized_shape, weight, bias, eps, p, training, bits, prenorm, generator)


def dropout_add_rms_norm_quantized(input: torch.Tensor, residual: torch.Tensor, normalized_shape: Union[int, Sequence[int]],
                                   weight: Optional[torch.Tensor] = None, eps: Optional[float] = None, p: float = 0.0, training: bool = True, bits: int = 4,
                                   prenorm: bool = False, generator: Optional[torch.Generator] = None):
    """:func:`dropout_add_layer_norm_quantized` for the RMS norm: ``rms_norm_quantized(dropout_add(input, residual, p, training), ...)`` as one node
    with one seed (pre-norm models: ``prenorm=True`` returns ``(y, h)``)."""
    return _dropout_add_norm_quantized(False, input, residual, normalized_shape, weight, None, eps, p, training, bits, prenorm, generator)


class _DropoutAddNorm:
    """What the two fused modules put in front of their quantized norm: ``p``, ``prenorm`` and a ``forward`` of two tensors."""

    def _configure(self, p: float, prenorm: bool):
        _check_p(p)
        self.p, self.prenorm = float(p), bool(prenorm)
        return self

    def forward(self, input: torch.Tensor, residual: torch.Tensor):
        bias = self.bias if self._centred else None
        if not self.training and kept.trains(input, residual, self.weight, bias):     # (eval: the dropout is off, torch's exact gradients on residual + input)
            h = residual + input
            y = _torch_norm(self._centred, h, self.normalized_shape, self.weight, bias, self.eps)
            return (y, h) if self.prenorm else y
        return _dropout_add_norm_quantized(self._centred, input, residual, self.normalized_shape, self.weight, bias, self.eps, self.p, self.training, self.bits,
                                           self.prenorm, self.generator)

    def extra_repr(self) -> str:
        return f'{super().extra_repr()}, p={self.p}, prenorm={self.prenorm}'


class DropoutAddLayerNorm(_DropoutAddNorm, QuantizedLayerNorm):
    r"""``LayerNorm(residual + dropout(input))``, a post-norm sublayer's ending (``prenorm=True``: ``(y, h)`` with the sum that goes on), as one node
    on one launch forward and two backward (:func:`dropout_add_layer_norm_quantized`).  A :class:`QuantizedLayerNorm` whose ``forward`` takes
    ``(input, residual)``; parameters after the norm's: ``p`` (drop probability, default 0), ``prenorm``, ``bits``, ``generator``.  ``m.eval()``
    switches the dropout off; gradients asked for in eval mode are torch's exact ones on ``residual + input``.

        >>> m = fewbit.DropoutAddLayerNorm(768, eps=1e-12, p=0.1)
        >>> hidden = m(dense(hidden), residual)                       # LayerNorm(dropout(dense(x)) + residual)
    """

    def __init__(self, normalized_shape, eps: float = 1e-5, elementwise_affine: bool = True, bias: bool = True, device=None, dtype=None, p: float = 0.0,
                 prenorm: bool = False, bits: int = 4, generator: Optional[torch.Generator] = None) -> None:
        super().__init__(normalized_shape, eps, elementwise_affine, bias, device, dtype, bits, generator)
        self._configure(p, prenorm)

    @classmethod
    def from_layer_norm(cls, module: torch.nn.LayerNorm, p: float = 0.0, prenorm: bool = False, bits: int = 4,
                        generator: Optional[torch.Generator] = None) -> 'DropoutAddLayerNorm':
        """A ``DropoutAddLayerNorm`` that SHARES the parameters of ``module``"""
        return super().from_layer_norm(module, bits, generator)._configure(p, prenorm)


class DropoutAddRMSNorm(_DropoutAddNorm, QuantizedRMSNorm):
    r"""``RMSNorm(residual + dropout(input))`` as one node (:func:`dropout_add_rms_norm_quantized`); with ``prenorm=True``, the pre-norm block of the
    Llama / Mistral / Qwen / T5 family, ``forward`` returns ``(y, h)`` and ``h`` goes on as the residual stream.  A :class:`QuantizedRMSNorm` whose
    ``forward`` takes ``(input, residual)``; parameters after the norm's: ``p`` (default 0), ``prenorm``, ``bits``, ``generator``.

        >>> m = fewbit.DropoutAddRMSNorm(4096, eps=1e-6, prenorm=True)
        >>> normed, stream = m(attention_output, stream)
    """

    def __init__(self, normalized_shape, eps: Optional[float] = None, elementwise_affine: bool = True, device=None, dtype=None, p: float = 0.0,
                 prenorm: bool = False, bits: int = 4, generator: Optional[torch.Generator] = None) -> None:
        super().__init__(normalized_shape, eps, elementwise_affine, device, dtype, bits, generator)
        self._configure(p, prenorm)

    @classmethod
    def from_rms_norm(cls, module: torch.nn.Module, p: float = 0.0, prenorm: bool = False, bits: int = 4,
                      generator: Optional[torch.Generator] = None) -> 'DropoutAddRMSNorm':
        """A ``DropoutAddRMSNorm`` that SHARES the weight of ``module`` (what :meth:`QuantizedRMSNorm.from_rms_norm` accepts)"""
        return super().from_rms_norm(module, bits, generator)._configure(p, prenorm)
