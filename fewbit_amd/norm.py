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
           'dropout_add_rms_norm_quantized', 'DropoutAddRMSNorm', 'rms_norm_linear_mx', 'MXNormLinear', 'layer_norm_linear_mx', 'MXLayerNormLinear')

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


# ---- the RMS norm and the linears behind it on ONE set of MX cells: x^ kept once, for the norm's backward and for every weight gradient ------------------

def _seed_plus(seed, k: int):
    """seed + k of a call's one draw: an int, or a new device word while the stream is being captured"""
    return seed + k if isinstance(seed, torch.Tensor) else (seed + k) & 0xffffffffffffffff


def _fp32_product(g: torch.Tensor, xq: torch.Tensor) -> torch.Tensor:
    """``g^T xq`` with fp32 sums that are not rounded to a 16-bit dtype on the way (the caller scales the columns first and rounds once)"""
    if g.is_cuda and g.dtype != torch.float32:
        with torch.autocast('cuda', enabled=False):
            return torch.mm(g.T, xq, out_dtype=torch.float32)
    return g.T @ xq


def _linears_backward(ctx, cells, gamma, beta, weights, grads, need_gy: bool, first: int):
    """What the linears behind a norm on MX cells hand back, for both nodes below -> ``(gy, grad_weights, grad_biases)``: ``gy = sum_i G_i W_i`` in ONE
    buffer (None where ``need_gy`` is False or no gradient arrived), ``dW_i = (G_i^T x^q) * gamma`` by columns, plus ``(sum_rows G_i) (x) beta`` where
    the norm has a ``beta`` (the layer norm: ``y = x^ * gamma + beta``), formed in fp32 and rounded once; ``db_i = sum_rows G_i``, exact.  ``first``:
    the index of the first weight among the node's inputs."""
    (rows, width), count, format, needs = ctx.flat_shape, ctx.count, ctx.format, ctx.needs_input_grad
    grad_weights, grad_biases, gy, decoded = [None] * count, [None] * count, None, {}

    def xq(dtype):                                              # the decode route: x^q ONCE per dtype, a transient of the input's size
        if dtype not in decoded:
            decoded[dtype] = (cabi_x.mx_unpack(cells, rows, width, format, dtype) if ctx.native else
                              cabi_x.mx_unpack_host(cells.cpu(), rows, width, format).to(device=cells.device, dtype=dtype))
        return decoded[dtype]

    for i, (g, weight) in enumerate(zip(grads, weights)):
        if g is None:
            continue
        if need_gy:                                             # gy = sum_i G_i W_i in ONE buffer
            w = weight if weight.dtype == g.dtype else weight.to(g.dtype)          # (under autocast: the cast autocast makes itself)
            gy = g @ w if gy is None else gy.addmm_(g, w)
        want_bias = ctx.has_bias[i] and needs[first + count + i]
        if beta is None:
            if want_bias:
                grad_biases[i] = g.sum(dim=0)
            column_sum = None
        elif want_bias or needs[first + i]:                     # s = sum_rows G_i in fp32: db_i, and the rank-one term of dW_i
            column_sum = g.sum(dim=0, dtype=cabi_x._work_dtype(g))
            if want_bias:
                grad_biases[i] = column_sum.to(g.dtype)
        if needs[first + i]:
            fout = g.shape[1]
            if ctx.native and g.dtype in DTYPES and cabi_x.mx_wgrad_serves(rows, width, fout, format):
                packed = cabi_x.mx_pack(linear._unit_stride(g), _seed_plus(ctx.seed, 1 + i), 'fp8', 'grad')
                product = cabi_x.mx_wgrad(packed, cells, rows, width, fout, format, torch.float32)
            else:
                g2 = g if ctx.native and g.dtype in DTYPES else g.to(cabi_x._work_dtype(g))
                product = _fp32_product(g2, xq(g2.dtype))
            # dW = (G^T x^q) * gamma by columns: the fp32 product is a transient of the WEIGHT's size, rounded once
            product = product * gamma.detach().to(product.dtype)[None, :]
            if column_sum is not None:
                product = torch.addr(product, column_sum.to(product.dtype), beta.detach().to(product.dtype))
            grad_weights[i] = product.to(weight.dtype)
    return gy, grad_weights, grad_biases


class _RMSNormLinearMX(torch.autograd.Function):
    """``tuple(F.linear(F.rms_norm(input, gamma), W_i, b_i))`` as ONE node (:func:`rms_norm_linear_mx`).  Kept for backward: ONE uint8 buffer of
    ``cabi_x.mx_bytes(rows, width, format)`` bytes (the cells of the fp32 ``x^``), ``rstd`` (fp32 per row), gamma and the weights; ``y`` is not.  On
    ``ctx``: the call's ONE seed draw (an int; a device word while the stream is being captured): seed + 0 rounds the cells, seed + 1 + i the fp8
    pack of ``G_i``, so that no two roundings share a seed."""

    @staticmethod
    def forward(ctx, input, gamma, eps: float, format: str, generator, count: int, *parameters):
        weights, biases = parameters[:count], parameters[count:]
        flat = input.detach().reshape(-1, input.shape[-1])
        ctx.format, ctx.flat_shape, ctx.input_shape, ctx.input_dtype, ctx.count = format, tuple(flat.shape), input.shape, input.dtype, count
        ctx.has_bias = tuple(b is not None for b in biases)
        ctx.autocast = linear._autocast_seen(input.device.type)
        ctx.set_materialize_grads(False)
        ctx.native = (linear._kernels_take(flat) and 1 <= flat.shape[1] <= cabi_x.MX_NORM_MAX_WIDTH and gamma.device == flat.device
                      and gamma.dtype in DTYPES)
        if ctx.native:
            ctx.seed = linear._sketch_seed(generator, flat.device)
            y, cells, rstd = cabi_x.mx_rms_norm_forward(linear._unit_stride(flat), _as(gamma, flat.dtype), eps, format, _seed_plus(ctx.seed, 0))
        else:
            ctx.seed = linear._draw_seed(generator if generator is None or generator.device.type == 'cpu' else None)
            y, cells, rstd = cabi_x.mx_rms_norm_host(flat, gamma, eps, format, ctx.seed)
        ctx.save_for_backward(cells, rstd, gamma, *weights)
        y = y.view(input.shape)
        return tuple(F.linear(y, w, b) for w, b in zip(weights, biases))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grad_outputs):
        with linear._autocast_as(ctx.autocast):
            return _RMSNormLinearMX._backward(ctx, grad_outputs)

    @staticmethod
    def _backward(ctx, grad_outputs):
        cells, rstd, gamma, *weights = ctx.saved_tensors        # read once: a non-re-entrant checkpoint unpacks a saved tensor one time only
        (rows, width), count, format, needs = ctx.flat_shape, ctx.count, ctx.format, ctx.needs_input_grad
        grads = [None if g is None else linear._dense_rows(g).reshape(rows, -1) for g in grad_outputs]
        gy, grad_weights, grad_biases = _linears_backward(ctx, cells, gamma, None, weights, grads, needs[0] or needs[1], 6)
        grad_input = grad_gamma = None
        if gy is not None:
            want = (needs[0], needs[1])
            if ctx.native:
                gy = gy if gy.dtype in DTYPES else gy.float()
                dx, dgamma = cabi_x.mx_rms_norm_backward(gy, cells, rstd, _as(gamma, gy.dtype), format, want)
            else:
                dx, dgamma = cabi_x.mx_rms_norm_backward_host(gy, cells, rstd, gamma, format)
            grad_input = dx.to(ctx.input_dtype).view(ctx.input_shape) if want[0] else None
            grad_gamma = dgamma.to(gamma.dtype).view(gamma.shape) if want[1] else None
        return (grad_input, grad_gamma, None, None, None, None, *grad_weights, *grad_biases)


def _mx_kernels_take(flat: torch.Tensor, gamma: torch.Tensor) -> bool:
    """whether the kernels of fewbit_mxnorm.hip serve the rows of ``flat`` with ``gamma``"""
    return linear._kernels_take(flat) and 1 <= flat.shape[1] <= cabi_x.MX_NORM_MAX_WIDTH and gamma.device == flat.device and gamma.dtype in DTYPES


class _AddRMSNormLinearMX(torch.autograd.Function):
    """``tuple(F.linear(F.rms_norm(residual + dropout(input), gamma), W_i, b_i))`` as ONE node, with ``h = residual + dropout(input)`` behind the
    tuple where ``prenorm``.  Kept for backward: what :class:`_RMSNormLinearMX` keeps -- the cells, ``rstd``, gamma and the weights; neither a mask nor
    ``h``.  On ``ctx``: the call's ONE seed draw and ``p``: seed + 0 rounds the cells, seed + 1 + i the fp8 pack of ``G_i``, seed + 1 + count draws
    the mask."""

    @staticmethod
    def forward(ctx, input, residual, gamma, eps: float, format: str, generator, p: float, prenorm: bool, count: int, *parameters):
        weights, biases = parameters[:count], parameters[count:]
        flat, res = input.detach().reshape(-1, input.shape[-1]), residual.detach().reshape(-1, input.shape[-1])
        ctx.format, ctx.flat_shape, ctx.input_shape, ctx.input_dtype, ctx.count = format, tuple(flat.shape), input.shape, input.dtype, count
        ctx.has_bias, ctx.p, ctx.prenorm = tuple(b is not None for b in biases), p, prenorm
        ctx.autocast = linear._autocast_seen(input.device.type)
        ctx.set_materialize_grads(False)
        ctx.native = True                                       # (the caller has made sure that the kernels serve the call: rms_norm_linear_mx)
        ctx.seed = linear._sketch_seed(generator, flat.device)
        seeds = (_seed_plus(ctx.seed, 0), _seed_plus(ctx.seed, 1 + count))
        seeds = torch.cat(seeds) if isinstance(ctx.seed, torch.Tensor) else seeds           # (while capturing: the two device words side by side)
        y, cells, rstd, h = cabi_x.mx_add_rms_norm_forward(linear._unit_stride(flat), linear._unit_stride(res), _as(gamma, flat.dtype), eps, format, seeds, p, prenorm)
        ctx.save_for_backward(cells, rstd, gamma, *weights)
        y = y.view(input.shape)
        outputs = tuple(F.linear(y, w, b) for w, b in zip(weights, biases))
        return (*outputs, h.view(input.shape)) if prenorm else outputs

    @staticmethod
    @once_differentiable
    def backward(ctx, *grad_outputs):
        with linear._autocast_as(ctx.autocast):
            return _AddRMSNormLinearMX._backward(ctx, grad_outputs)

    @staticmethod
    def _backward(ctx, grad_outputs):
        cells, rstd, gamma, *weights = ctx.saved_tensors        # read once: a non-re-entrant checkpoint unpacks a saved tensor one time only
        (rows, width), count, format, needs = ctx.flat_shape, ctx.count, ctx.format, ctx.needs_input_grad
        grads = [None if g is None else linear._dense_rows(g).reshape(rows, -1) for g in grad_outputs]
        at_h = grads.pop() if ctx.prenorm else None             # the gradient that arrives at the sum: it goes into the kernel as gh
        gy, grad_weights, grad_biases = _linears_backward(ctx, cells, gamma, None, weights, grads, any(needs[:3]), 9)
        if gy is None and at_h is not None and (needs[0] or needs[1]):
            gy = torch.zeros_like(at_h)                         # (nothing arrived at a linear: the norm hands on 0, to which at_h is added and masked)
        grad_input = grad_residual = grad_gamma = None
        if gy is not None:
            want = (needs[1], needs[0], needs[2])               # (dres: the residual's gradient; dbranch: the input's)
            gy = gy if gy.dtype in DTYPES else gy.float()
            gy = gy if at_h is None or at_h.dtype == gy.dtype else gy.to(at_h.dtype)        # (under autocast: h has the input's dtype)
            dres, dbranch, dgamma = cabi_x.mx_add_rms_norm_backward(gy, cells, rstd, _as(gamma, gy.dtype), format, _seed_plus(ctx.seed, 1 + count), ctx.p, at_h, want)
            grad_input = dbranch.to(ctx.input_dtype).view(ctx.input_shape) if want[1] else None
            grad_residual = dres.to(ctx.input_dtype).view(ctx.input_shape) if want[0] else None
            grad_gamma = dgamma.to(gamma.dtype).view(gamma.shape) if want[2] else None
        return (grad_input, grad_residual, grad_gamma, None, None, None, None, None, None, *grad_weights, *grad_biases)


def rms_norm_linear_mx(input: torch.Tensor, norm_weight: torch.Tensor, weights: Sequence[torch.Tensor], biases: Optional[Sequence[Optional[torch.Tensor]]] = None,
                       eps: Optional[float] = None, format: str = 'fp4', generator: Optional[torch.Generator] = None,
                       residual: Optional[torch.Tensor] = None, p: float = 0.0, training: bool = True, prenorm: bool = False) -> tuple:
    """``tuple(F.linear(F.rms_norm(input, (width, ), norm_weight, eps), W, b) for W, b in zip(weights, biases))`` as ONE node that keeps ONE buffer for
    all of it: the normalized rows ``x^ = x * rstd`` as MXFP4 (``format='fp4'``) or MXFP6 (``'fp6'``) cells down their columns, one fp32 ``rstd``
    per row, ``norm_weight`` and the weights -- at width 4096 and fp4 2180 bytes a token, where ``QuantizedRMSNorm(bits=4)`` in front of three
    ``MXLinear`` keeps 9088.  The output of the norm is not kept: because ``y = x^ * gamma``, ``dW_i = G_i^T y = (G_i^T x^) * gamma`` by columns.

    * Forward: one kernel (``cabi_x.mx_rms_norm_forward``) writes ``y``, ``rstd`` and the cells of the FP32 ``x^``; then ``F.linear`` per weight.
    * Backward: ``gy = sum_i G_i W_i`` in one buffer; ``dW_i`` from ``cabi_x.mx_wgrad`` on the fp8 cells of ``G_i`` and the kept cells (where
      ``cabi_x.mx_wgrad_serves`` denies -- widths that are no multiples of 32 -- a decode and a GEMM), as fp32 sums that are scaled by
      ``norm_weight`` and rounded once: an fp32 transient of the weight's size, not of the tokens'.  ``db_i`` is exact.  ``dx`` and the gradient
      of ``norm_weight`` come from ``cabi_x.mx_rms_norm_backward`` on the decoded cells: ``E[x^q] = x^``, so ``E[dW_i] = G_i^T y``; ``dx`` is
      not linear in ``x^q`` and carries a bias of second order in the rounding, as the quantized norms' does.
    * Seeds: ONE draw from ``linear._sketch_seed`` per call; the cells take it plus 0, the fp8 rounding of ``G_i`` plus 1 + i.
    * Widths above 8192, host tensors and float64 take the host route: the same definitions on ``cabi_x.mx_pack_host``.
    * Grad mode off, or nothing that requires grad: plain ``F.rms_norm`` and ``F.linear``; no seed is drawn, nothing is kept.
    * ``eps=None`` means ``torch.finfo(input.dtype).eps``, as in :func:`rms_norm_quantized`.  Under ``torch.autocast`` the norm runs in the input's
      dtype and the linears as autocast casts them; backward runs under the state the forward saw.
    * ``residual`` (of the input's shape): the norm reads ``h = residual + dropout(input, p, training)``, a sublayer's entry, still as ONE node with
      ONE seed draw (the mask takes it plus 1 + the number of weights) on one launch forward (``cabi_x.mx_add_rms_norm_forward``); backward adds
      the gradient arriving at ``h`` and applies the mask inside the norm's kernel.  Kept: the same tensors -- no mask and not ``h``.  With
      ``prenorm=True`` ``h`` is the LAST element of the returned tuple (the residual stream that goes on).  The values are bit for bit those of
      :func:`fewbit.functional.dropout_add` followed by this function.  A mask at a width that is no multiple of 8, widths above 8192, host
      tensors, float64, a residual of another dtype or device and ``use_native_sketch(False)`` ARE that composition (two nodes, two seeds)."""
    linear._check_mx_format(format)
    weights = tuple(weights)
    biases = (None, ) * len(weights) if biases is None else tuple(biases)
    if len(biases) != len(weights) or not weights:
        raise ValueError(f'{len(weights)} weights and {len(biases)} biases: one bias (or None) per weight is needed, and at least one weight')
    eps = float(torch.finfo(input.dtype).eps if eps is None else eps)
    if residual is None:
        if not kept.trains(input, norm_weight, *weights, *biases) or input.numel() == 0:
            y = F.rms_norm(input, (input.shape[-1], ), norm_weight, eps)
            return tuple(F.linear(y, w, b) for w, b in zip(weights, biases))
        return _RMSNormLinearMX.apply(input, norm_weight, eps, format, generator, len(weights), *weights, *biases)
    _check_p(p)
    if tuple(residual.shape) != tuple(input.shape):
        raise ValueError(f'residual should have the shape of input, {tuple(input.shape)}, but got {tuple(residual.shape)}.')
    p = float(p) if training else 0.0
    trains = kept.trains(input, residual, norm_weight, *weights, *biases) and input.numel() != 0
    flat = input.detach().reshape(-1, input.shape[-1]) if trains else None
    if (not trains or not _mx_kernels_take(flat, norm_weight) or residual.dtype != input.dtype or residual.device != input.device
            or (cabi_x.dropout_threshold(p) > 0 and flat.shape[1] % 8 != 0)):
        # nothing trains (plain torch behind the sum), or the kernels do not serve the call: the composition, whose second half is the call without a residual
        h = dropout_add(input, residual, p, training, generator)
        outputs = rms_norm_linear_mx(h, norm_weight, weights, biases, eps, format, generator)
        return (*outputs, h) if prenorm else outputs
    return _AddRMSNormLinearMX.apply(input, residual, norm_weight, eps, format, generator, p, bool(prenorm), len(weights), *weights, *biases)


class MXNormLinear(torch.nn.Module):
    r"""An RMS norm and the linear layers that read its output -- q / k / v behind the norm at the head of an attention block -- as one module that
    keeps ONE set of MXFP4 / MXFP6 cells for all of them (:func:`rms_norm_linear_mx`); ``forward`` returns the tuple of the linears' outputs.  The
    linears are plain ``nn.Linear`` layers in ``self.linears``, the norm's weight is ``self.weight``.  In ``eval()`` mode gradients are torch's exact
    ones and nothing is kept.  ``forward(input, residual)`` normalizes ``residual + dropout(input, p)`` in the same node (``p``, ``prenorm``: as in
    :func:`rms_norm_linear_mx`; with ``prenorm=True`` the sum is the last element of the tuple).

        >>> m = fewbit.MXNormLinear(64, [(64, 96, False), (64, 32, False), (64, 32, False)], eps=1e-6)
        >>> q, k, v = m(torch.randn(128, 64))
        >>> q, k, v, stream = fewbit.MXNormLinear(64, [(64, 64, False)] * 3, p=0.1, prenorm=True)(mlp_output, stream)
        >>> m = fewbit.MXNormLinear.from_modules(block.input_layernorm, [attn.q_proj, attn.k_proj, attn.v_proj], format='fp4')
    """

    def __init__(self, norm_weight_shape, linears, eps: Optional[float] = None, format: str = 'fp4', generator: Optional[torch.Generator] = None,
                 device=None, dtype=None, p: float = 0.0, prenorm: bool = False) -> None:
        linear._check_mx_format(format)
        _check_p(p)
        super().__init__()
        self.p, self.prenorm = float(p), bool(prenorm)
        width = norm_weight_shape if isinstance(norm_weight_shape, int) else math.prod(norm_weight_shape)
        self.weight = torch.nn.Parameter(torch.ones(width, device=device, dtype=dtype))
        self.linears = torch.nn.ModuleList(torch.nn.Linear(fin, fout, bias, device=device, dtype=dtype) for fin, fout, bias in linears)
        if any(m.in_features != width for m in self.linears):
            raise ValueError(f'every linear must read the {width} features of the norm')
        self.eps, self.format, self.generator = eps, format, generator

    @classmethod
    def from_modules(cls, norm: torch.nn.Module, linears: Sequence[torch.nn.Linear], format: str = 'fp4',
                     generator: Optional[torch.Generator] = None, p: float = 0.0, prenorm: bool = False) -> 'MXNormLinear':
        """An ``MXNormLinear`` that SHARES the weight of ``norm`` -- a ``torch.nn.RMSNorm``, or any module with a 1-D ``weight`` and a float
        ``variance_epsilon`` or ``eps`` -- and the given ``nn.Linear`` modules themselves"""
        weight, eps = getattr(norm, 'weight', None), getattr(norm, 'variance_epsilon', getattr(norm, 'eps', None))
        if not isinstance(weight, torch.Tensor) or weight.dim() != 1 or not (eps is None or isinstance(eps, float)):
            raise TypeError(f'{type(norm).__name__} has no 1-D weight with a float variance_epsilon or eps')
        new = cls(weight.numel(), [], eps, format, generator, device='meta', p=p, prenorm=prenorm)
        new.weight, new.linears = weight, torch.nn.ModuleList(linears)
        return new.train(norm.training)

    def forward(self, input: torch.Tensor, residual: Optional[torch.Tensor] = None) -> tuple:
        weights, biases = [m.weight for m in self.linears], [m.bias for m in self.linears]
        if not self.training:                                   # (eval: the dropout is off, torch's exact gradients on residual + input)
            eps = float(torch.finfo(input.dtype).eps if self.eps is None else self.eps)
            h = input if residual is None else residual + input
            y = F.rms_norm(h, (h.shape[-1], ), self.weight, eps)
            outputs = tuple(F.linear(y, w, b) for w, b in zip(weights, biases))
            return (*outputs, h) if residual is not None and self.prenorm else outputs
        return rms_norm_linear_mx(input, self.weight, weights, biases, self.eps, self.format, self.generator, residual, self.p, True, self.prenorm)

    def extra_repr(self) -> str:
        return f'{self.weight.numel()}, eps={self.eps}, format={self.format}' + (f', p={self.p}, prenorm={self.prenorm}' if self.p or self.prenorm else '')


# ---- the LAYER norm and the linears behind it on ONE set of MX cells: y = x^ * gamma + beta, so dW_i takes one rank-one term in beta more -----------------

class _LayerNormLinearMX(torch.autograd.Function):
    """``tuple(F.linear(F.layer_norm(input, gamma, beta), W_i, b_i))`` as ONE node (:func:`layer_norm_linear_mx`), with the norm's output in front where
    ``return_normed``.  Kept for backward: ONE uint8 buffer of ``cabi_x.mx_bytes(rows, width, format)`` bytes (the cells of the fp32 ``x^``), ``rstd``
    (fp32 per row), gamma, beta and the weights; ``y``, the mean and the input are not.  Seeds as in :class:`_RMSNormLinearMX`."""

    @staticmethod
    def forward(ctx, input, gamma, beta, eps: float, format: str, generator, return_normed: bool, count: int, *parameters):
        weights, biases = parameters[:count], parameters[count:]
        flat = input.detach().reshape(-1, input.shape[-1])
        ctx.format, ctx.flat_shape, ctx.input_shape, ctx.input_dtype, ctx.count = format, tuple(flat.shape), input.shape, input.dtype, count
        ctx.has_bias, ctx.has_beta, ctx.return_normed = tuple(b is not None for b in biases), beta is not None, return_normed
        ctx.autocast = linear._autocast_seen(input.device.type)
        ctx.set_materialize_grads(False)
        ctx.native = (linear._kernels_take(flat) and 1 <= flat.shape[1] <= cabi_x.MX_NORM_MAX_WIDTH and gamma.dtype in DTYPES
                      and all(p.device == flat.device for p in (gamma, beta) if p is not None) and (beta is None or beta.dtype in DTYPES))
        if ctx.native:
            ctx.seed = linear._sketch_seed(generator, flat.device)
            y, cells, rstd, _ = cabi_x.mx_layer_norm_forward(linear._unit_stride(flat), _as(gamma, flat.dtype), _as(beta, flat.dtype), eps, format,
                                                             _seed_plus(ctx.seed, 0))
        else:
            ctx.seed = linear._draw_seed(generator if generator is None or generator.device.type == 'cpu' else None)
            y, cells, rstd, _ = cabi_x.mx_layer_norm_host(flat, gamma, beta, eps, format, ctx.seed)
        ctx.save_for_backward(cells, rstd, gamma, *(() if beta is None else (beta, )), *weights)
        y = y.view(input.shape)
        outputs = tuple(F.linear(y, w, b) for w, b in zip(weights, biases))
        return (y, *outputs) if return_normed else outputs

    @staticmethod
    @once_differentiable
    def backward(ctx, *grad_outputs):
        with linear._autocast_as(ctx.autocast):
            return _LayerNormLinearMX._backward(ctx, grad_outputs)

    @staticmethod
    def _backward(ctx, grad_outputs):
        cells, rstd, gamma, *rest = ctx.saved_tensors           # read once: a non-re-entrant checkpoint unpacks a saved tensor one time only
        beta, weights = (rest[0], rest[1:]) if ctx.has_beta else (None, rest)
        (rows, width), count, format, needs = ctx.flat_shape, ctx.count, ctx.format, ctx.needs_input_grad
        grads = [None if g is None else linear._dense_rows(g).reshape(rows, -1) for g in grad_outputs]
        at_y = grads.pop(0) if ctx.return_normed else None      # the gradient that arrives at the norm's own output
        gy, grad_weights, grad_biases = _linears_backward(ctx, cells, gamma, beta, weights, grads, any(needs[:3]), 8)
        if at_y is not None and any(needs[:3]):
            gy = at_y if gy is None else gy.add_(at_y) if gy.dtype == at_y.dtype else gy + at_y
        grad_input = grad_gamma = grad_beta = None
        if gy is not None:
            want = (needs[0], needs[1], ctx.has_beta and needs[2])
            if ctx.native:
                gy = gy if gy.dtype in DTYPES else gy.float()
                dx, dgamma, dbeta = cabi_x.mx_layer_norm_backward(linear._unit_stride(gy), cells, rstd, _as(gamma, gy.dtype), format, want)
            else:
                dx, dgamma, dbeta = cabi_x.mx_layer_norm_backward_host(gy, cells, rstd, gamma, format)
            grad_input = dx.to(ctx.input_dtype).view(ctx.input_shape) if want[0] else None
            grad_gamma = dgamma.to(gamma.dtype).view(gamma.shape) if want[1] else None
            grad_beta = dbeta.to(beta.dtype).view(beta.shape) if want[2] else None
        return (grad_input, grad_gamma, grad_beta, None, None, None, None, None, *grad_weights, *grad_biases)


class _AddLayerNormLinearMX(torch.autograd.Function):
    """``tuple(F.linear(F.layer_norm(residual + dropout(input), gamma, beta), W_i, b_i))`` as ONE node, with the norm's output in front where
    ``return_normed`` and ``h = residual + dropout(input)`` behind the tuple where ``prenorm``.  Kept for backward: what :class:`_LayerNormLinearMX`
    keeps -- the cells, ``rstd``, gamma, beta and the weights; neither a mask nor ``h`` nor ``y``.  On ``ctx``: the call's ONE seed draw and ``p``:
    seed + 0 rounds the cells, seed + 1 + i the fp8 pack of ``G_i``, seed + 1 + count draws the mask."""

    @staticmethod
    def forward(ctx, input, residual, gamma, beta, eps: float, format: str, generator, return_normed: bool, p: float, prenorm: bool, count: int, *parameters):
        weights, biases = parameters[:count], parameters[count:]
        flat, res = input.detach().reshape(-1, input.shape[-1]), residual.detach().reshape(-1, input.shape[-1])
        ctx.format, ctx.flat_shape, ctx.input_shape, ctx.input_dtype, ctx.count = format, tuple(flat.shape), input.shape, input.dtype, count
        ctx.has_bias, ctx.has_beta, ctx.return_normed = tuple(b is not None for b in biases), beta is not None, return_normed
        ctx.p, ctx.prenorm = p, prenorm
        ctx.autocast = linear._autocast_seen(input.device.type)
        ctx.set_materialize_grads(False)
        ctx.native = True                                       # (the caller has made sure that the kernels serve the call: layer_norm_linear_mx)
        ctx.seed = linear._sketch_seed(generator, flat.device)
        seeds = (_seed_plus(ctx.seed, 0), _seed_plus(ctx.seed, 1 + count))
        seeds = torch.cat(seeds) if isinstance(ctx.seed, torch.Tensor) else seeds           # (while capturing: the two device words side by side)
        y, cells, rstd, h, _ = cabi_x.mx_add_layer_norm_forward(linear._unit_stride(flat), linear._unit_stride(res), _as(gamma, flat.dtype),
                                                                _as(beta, flat.dtype), eps, format, seeds, p, prenorm)
        ctx.save_for_backward(cells, rstd, gamma, *(() if beta is None else (beta, )), *weights)
        y = y.view(input.shape)
        outputs = tuple(F.linear(y, w, b) for w, b in zip(weights, biases))
        return (*((y, ) if return_normed else ()), *outputs, *((h.view(input.shape), ) if prenorm else ()))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grad_outputs):
        with linear._autocast_as(ctx.autocast):
            return _AddLayerNormLinearMX._backward(ctx, grad_outputs)

    @staticmethod
    def _backward(ctx, grad_outputs):
        cells, rstd, gamma, *rest = ctx.saved_tensors           # read once: a non-re-entrant checkpoint unpacks a saved tensor one time only
        beta, weights = (rest[0], rest[1:]) if ctx.has_beta else (None, rest)
        (rows, width), count, format, needs = ctx.flat_shape, ctx.count, ctx.format, ctx.needs_input_grad
        grads = [None if g is None else linear._dense_rows(g).reshape(rows, -1) for g in grad_outputs]
        at_y = grads.pop(0) if ctx.return_normed else None      # the gradient that arrives at the norm's own output: into the kernel as gy_add
        at_h = grads.pop() if ctx.prenorm else None             # the gradient that arrives at the sum: into the kernel as gh
        gy, grad_weights, grad_biases = _linears_backward(ctx, cells, gamma, beta, weights, grads, any(needs[:4]), 11)
        if not any(needs[:4]):
            at_y = at_h = None
        if gy is None and at_y is not None:
            gy, at_y = at_y, None                               # (nothing arrived at a linear: what arrived at y is gy itself)
        if gy is None and at_h is not None and (needs[0] or needs[1]):
            gy = torch.zeros_like(at_h)                         # (nothing arrived at the norm: it hands on 0, to which at_h is added and masked)
        grad_input = grad_residual = grad_gamma = grad_beta = None
        if gy is not None:
            want = (needs[1], needs[0], needs[2], ctx.has_beta and needs[3])        # (dres: the residual's gradient; dbranch: the input's)
            gy = gy if gy.dtype in DTYPES else gy.float()
            other = at_y if at_y is not None else at_h
            gy = gy if other is None or other.dtype == gy.dtype else gy.to(other.dtype)     # (under autocast: y and h have the input's dtype)
            dres, dbranch, dgamma, dbeta = cabi_x.mx_add_layer_norm_backward(linear._unit_stride(gy), cells, rstd, _as(gamma, gy.dtype), format,
                                                                             _seed_plus(ctx.seed, 1 + count), ctx.p, at_h, want, at_y)
            grad_input = dbranch.to(ctx.input_dtype).view(ctx.input_shape) if want[1] else None
            grad_residual = dres.to(ctx.input_dtype).view(ctx.input_shape) if want[0] else None
            grad_gamma = dgamma.to(gamma.dtype).view(gamma.shape) if want[2] else None
            grad_beta = dbeta.to(beta.dtype).view(beta.shape) if want[3] else None
        return (grad_input, grad_residual, grad_gamma, grad_beta, None, None, None, None, None, None, None, *grad_weights, *grad_biases)


def _layer_norm_kernels_take(flat: torch.Tensor, gamma: torch.Tensor, beta: Optional[torch.Tensor]) -> bool:
    """whether the kernels of fewbit_mxlnorm.hip serve the rows of ``flat`` with ``gamma`` and ``beta`` (what makes :class:`_LayerNormLinearMX` native)"""
    return (_mx_kernels_take(flat, gamma) and (beta is None or (beta.device == flat.device and beta.dtype in DTYPES)))


def layer_norm_linear_mx(input: torch.Tensor, norm_weight: torch.Tensor, norm_bias: Optional[torch.Tensor], weights: Sequence[torch.Tensor],
                         biases: Optional[Sequence[Optional[torch.Tensor]]] = None, eps: float = 1e-5, format: str = 'fp4',
                         generator: Optional[torch.Generator] = None, return_normed: bool = False,
                         residual: Optional[torch.Tensor] = None, p: float = 0.0, training: bool = True, prenorm: bool = False) -> tuple:
    """``tuple(F.linear(F.layer_norm(input, (width, ), norm_weight, norm_bias, eps), W, b) for W, b in zip(weights, biases))`` as ONE node that keeps
    ONE buffer for all of it: the normalized rows ``x^ = (x - mean) * rstd`` as MXFP4 (``format='fp4'``) or MXFP6 (``'fp6'``) cells down their columns,
    one fp32 ``rstd`` per row, ``norm_weight``, ``norm_bias`` and the weights.  Neither the norm's output, nor the mean, nor the input is kept: because
    ``y = x^ * gamma + beta``, ``dW_i = G_i^T y = (G_i^T x^) * gamma`` by columns ``+ (sum_rows G_i) (x) beta``, and ``sum_rows G_i`` is ``db_i``.

    * ``return_normed=True`` puts ``y`` itself in front of the tuple (the post-norm case: in BERT / RoBERTa a LayerNorm output feeds the next linears
      AND the next residual); the gradient that arrives at it is added into ``gy = sum_i G_i W_i`` before the norm's backward.
    * Forward: one kernel (``cabi_x.mx_layer_norm_forward``) writes ``y``, ``rstd`` and the cells of the FP32 ``x^``; then ``F.linear`` per weight.
    * Backward: ``dW_i`` from ``cabi_x.mx_wgrad`` on the fp8 cells of ``G_i`` and the kept cells (where ``cabi_x.mx_wgrad_serves`` denies -- widths
      that are no multiples of 32 -- a decode and a GEMM), scaled by ``norm_weight``, plus ``s (x) norm_bias`` with ``s = G_i.sum(0)`` in fp32 (absent
      where ``norm_bias`` is None), formed in fp32 and rounded once.  ``db_i = s`` is exact.  ``dx`` and the gradients of ``norm_weight`` and
      ``norm_bias`` come from ``cabi_x.mx_layer_norm_backward``: ``E[x^q] = x^``, so ``E[dW_i] = G_i^T y``; the gradient of ``norm_bias`` does
      not read the cells; ``dx`` carries a bias of second order in the rounding, as the quantized norms' does.
    * Seeds: ONE draw from ``linear._sketch_seed`` per call; the cells take it plus 0, the fp8 rounding of ``G_i`` plus 1 + i.
    * Widths above 8192, host tensors and float64 take the host route: the same definitions on ``cabi_x.mx_pack_host``.
    * Grad mode off, or nothing that requires grad: plain ``F.layer_norm`` and ``F.linear``; no seed is drawn, nothing is kept.
    * Under ``torch.autocast`` the norm runs in the input's dtype and the linears as autocast casts them; backward runs under the state the forward
      saw.
    * ``residual`` (of the input's shape): the norm reads ``h = residual + dropout(input, p, training)`` -- every BERT / RoBERTa sublayer's end,
      ``LayerNorm(dropout(dense(x)) + input)`` -- still as ONE node with ONE seed draw (the mask takes it plus 1 + the number of weights) on one
      launch forward (``cabi_x.mx_add_layer_norm_forward``); backward adds the gradients arriving at ``y`` and at ``h`` and applies the mask inside
      the norm's kernel.  Kept: the same tensors -- no mask, not ``h``, not ``y``.  With ``prenorm=True`` ``h`` is the LAST element of the returned
      tuple (GPT-2 / ViT / OPT: the residual stream that goes on): ``(y if return_normed, *outputs, h if prenorm)``.  The values are bit for bit
      those of :func:`fewbit.functional.dropout_add` followed by this function.  A mask at a width that is no multiple of 8, widths above 8192,
      host tensors, float64, a residual of another dtype or device, ``use_native_sketch(False)`` and a call in which nothing trains ARE that
      composition (two nodes, two seeds)."""
    linear._check_mx_format(format)
    weights = tuple(weights)
    biases = (None, ) * len(weights) if biases is None else tuple(biases)
    if len(biases) != len(weights) or not weights:
        raise ValueError(f'{len(weights)} weights and {len(biases)} biases: one bias (or None) per weight is needed, and at least one weight')
    if residual is None:
        if not kept.trains(input, norm_weight, norm_bias, *weights, *biases) or input.numel() == 0:
            y = F.layer_norm(input, (input.shape[-1], ), norm_weight, norm_bias, float(eps))
            outputs = tuple(F.linear(y, w, b) for w, b in zip(weights, biases))
            return (y, *outputs) if return_normed else outputs
        return _LayerNormLinearMX.apply(input, norm_weight, norm_bias, float(eps), format, generator, bool(return_normed), len(weights), *weights, *biases)
    _check_p(p)
    if tuple(residual.shape) != tuple(input.shape):
        raise ValueError(f'residual should have the shape of input, {tuple(input.shape)}, but got {tuple(residual.shape)}.')
    p = float(p) if training else 0.0
    trains = kept.trains(input, residual, norm_weight, norm_bias, *weights, *biases) and input.numel() != 0
    flat = input.detach().reshape(-1, input.shape[-1]) if trains else None
    if (not trains or not _layer_norm_kernels_take(flat, norm_weight, norm_bias) or residual.dtype != input.dtype or residual.device != input.device
            or (cabi_x.dropout_threshold(p) > 0 and flat.shape[1] % 8 != 0)):
        # nothing trains (plain torch behind the sum), or the kernels do not serve the call: the composition, whose second half is the call without a residual
        h = dropout_add(input, residual, p, training, generator)
        outputs = layer_norm_linear_mx(h, norm_weight, norm_bias, weights, biases, eps, format, generator, return_normed)
        return (*outputs, h) if prenorm else outputs
    return _AddLayerNormLinearMX.apply(input, residual, norm_weight, norm_bias, float(eps), format, generator, bool(return_normed), p, bool(prenorm),
                                       len(weights), *weights, *biases)


class MXLayerNormLinear(torch.nn.Module):
    r"""A LayerNorm and the linear layers that read its output -- q / k / v of a BERT / RoBERTa / GPT-2 / ViT block, or the intermediate dense behind
    the attention output's LayerNorm -- as one module that keeps ONE set of MXFP4 / MXFP6 cells for all of them (:func:`layer_norm_linear_mx`);
    ``forward`` returns the tuple of the linears' outputs, with the norm's own output in front where ``return_normed`` (it also feeds the next
    residual there).  The linears are plain ``nn.Linear`` layers in ``self.linears``, the norm's parameters ``self.weight`` and ``self.bias``.  In
    ``eval()`` mode gradients are torch's exact ones and nothing is kept.  ``forward(input, residual)`` normalizes ``residual + dropout(input, p)`` in
    the same node (``p``, ``prenorm``: as in :func:`layer_norm_linear_mx`; with ``prenorm=True`` the sum is the last element of the tuple).

        >>> m = fewbit.MXLayerNormLinear(768, [(768, 768, True)] * 3)
        >>> q, k, v = m(torch.randn(128, 768))
        >>> m = fewbit.MXLayerNormLinear.from_modules(layer.attention.output.LayerNorm, [layer.intermediate.dense], return_normed=True)
        >>> y, h = m(hidden)
        >>> m = fewbit.MXLayerNormLinear.from_modules(layer.attention.output.LayerNorm, [layer.intermediate.dense], return_normed=True, p=0.1)
        >>> y, h = m(layer.attention.output.dense(context), hidden)            # LayerNorm(dropout(dense(context)) + hidden) and the dense behind it
    """

    def __init__(self, width: int, linears, eps: float = 1e-5, bias: bool = True, format: str = 'fp4', generator: Optional[torch.Generator] = None,
                 return_normed: bool = False, device=None, dtype=None, p: float = 0.0, prenorm: bool = False) -> None:
        linear._check_mx_format(format)
        _check_p(p)
        super().__init__()
        self.p, self.prenorm = float(p), bool(prenorm)
        self.weight = torch.nn.Parameter(torch.ones(width, device=device, dtype=dtype))
        self.register_parameter('bias', torch.nn.Parameter(torch.zeros(width, device=device, dtype=dtype)) if bias else None)
        self.linears = torch.nn.ModuleList(torch.nn.Linear(fin, fout, b, device=device, dtype=dtype) for fin, fout, b in linears)
        if any(m.in_features != width for m in self.linears):
            raise ValueError(f'every linear must read the {width} features of the norm')
        self.eps, self.format, self.generator, self.return_normed = eps, format, generator, return_normed

    @classmethod
    def from_modules(cls, norm: torch.nn.LayerNorm, linears: Sequence[torch.nn.Linear], format: str = 'fp4', generator: Optional[torch.Generator] = None,
                     return_normed: bool = False, p: float = 0.0, prenorm: bool = False) -> 'MXLayerNormLinear':
        """An ``MXLayerNormLinear`` that SHARES the weight and the bias of ``norm`` -- a ``torch.nn.LayerNorm`` over the last dimension with affine
        parameters -- and the given ``nn.Linear`` modules themselves"""
        weight, bias = getattr(norm, 'weight', None), getattr(norm, 'bias', None)
        if not isinstance(weight, torch.Tensor) or weight.dim() != 1 or not isinstance(getattr(norm, 'eps', None), float):
            raise TypeError(f'{type(norm).__name__} has no 1-D weight with a float eps')
        new = cls(weight.numel(), [], norm.eps, False, format, generator, return_normed, device='meta', p=p, prenorm=prenorm)
        new.weight, new.bias, new.linears = weight, bias, torch.nn.ModuleList(linears)
        return new.train(norm.training)

    def forward(self, input: torch.Tensor, residual: Optional[torch.Tensor] = None) -> tuple:
        weights, biases = [m.weight for m in self.linears], [m.bias for m in self.linears]
        if not self.training:                                   # (eval: the dropout is off, torch's exact gradients on residual + input)
            h = input if residual is None else residual + input
            y = F.layer_norm(h, (h.shape[-1], ), self.weight, self.bias, self.eps)
            outputs = tuple(F.linear(y, w, b) for w, b in zip(weights, biases))
            outputs = (y, *outputs) if self.return_normed else outputs
            return (*outputs, h) if residual is not None and self.prenorm else outputs
        return layer_norm_linear_mx(input, self.weight, self.bias, weights, biases, self.eps, self.format, self.generator, self.return_normed, residual,
                                    self.p, True, self.prenorm)

    def extra_repr(self) -> str:
        return (f'{self.weight.numel()}, eps={self.eps}, format={self.format}, return_normed={self.return_normed}'
                + (f', p={self.p}, prenorm={self.prenorm}' if self.p or self.prenorm else ''))
