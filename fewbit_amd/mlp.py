"""The plain MLP of the LayerNorm models (BERT / RoBERTa, GPT-2, ViT, OPT), ``fc2(act(fc1(x)))``, as ONE node on the row blocks of a seed:
:func:`mlp_mx` / :class:`MXMLP`.  ``x`` and the pre-activation ``u = fc1(x)`` are kept as MXFP4 / MXFP6 cells down their columns (:func:`linear_mx`
keeps its input so) and nothing else; both weight gradients are ``cabi_x.mx_wgrad`` calls on the scaled matrix instruction of gfx950 with nothing
decoded.  The gated MLP of the Llama family has the same shape of node in fewbit_amd/glu.py (``_GatedMLPMX``), whose seeds, keep and decode helpers
serve here; the activation kernels are fewbit_amd/csrc/fewbit_mxact.hip."""
import math
from typing import Optional

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import cabi_x, kept, linear
from .cabi import DTYPES
from .glu import _mx_decoded, _mx_keep, _mx_seeds

__all__ = ('mlp_mx', 'MXMLP')

ACTIVATIONS = cabi_x.MX_ACTIVATIONS

# the tensors one call rounds, in the order of their seeds: seed i is the call's ONE draw plus i.  No two of one role ('kept': x, u, product; 'grad':
# the others) share a seed
MLP_MX_SEEDS = ('x', 'u', 'd_u', 'product', 'grad_output')


def _check(activation: str, format: str) -> None:
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation should be one of {', '.join(map(repr, ACTIVATIONS))}, but got {activation!r}.")
    if format not in linear.MX_KEPT_FORMATS:
        raise ValueError(f"format should be 'fp4' or 'fp6', but got {format!r}.")


def _torch_act(u: torch.Tensor, activation: str) -> torch.Tensor:
    if activation == 'relu':
        return F.relu(u)
    if activation == 'silu':
        return F.silu(u)
    return F.gelu(u, approximate='tanh' if activation == 'gelu_tanh' else 'none')


def _slope(u: torch.Tensor, activation: str) -> torch.Tensor:
    """``act'`` of the definition: relu ``u > 0``; silu ``s (1 + u (1 - s))``; gelu ``Phi(u) + u phi(u)``; the tanh form ``s (1 + u (1 - s) 2 z')`` with
    ``s = sigmoid(2 z)``, ``z = sqrt(2 / pi) (u + 0.044715 u^3)``"""
    if activation == 'relu':
        return (u > 0).to(u.dtype)
    if activation == 'silu':
        s = torch.sigmoid(u)
        return s * (1 + u * (1 - s))
    if activation == 'gelu':
        return 0.5 * (1 + torch.erf(u * math.sqrt(0.5))) + u * torch.exp(-0.5 * u * u) * (1 / math.sqrt(2 * math.pi))
    k = math.sqrt(2 / math.pi)
    s = torch.sigmoid(2 * k * (u + 0.044715 * u**3))
    return s * (1 + u * (1 - s) * (2 * k * (1 + 3 * 0.044715 * u * u)))


def _serves(flat: torch.Tensor, u: torch.Tensor, out_features: int, format: str) -> bool:
    """whether the kernels of fewbit_mxact.hip and ``mx_wgrad`` take a call: ``flat`` the rows of ``x``, ``u`` the rows of ``fc1(x)``"""
    (rows, hidden), width = flat.shape, u.shape[-1]
    return (linear._kernels_take(u) and flat.dtype == u.dtype and u.dtype != torch.float32 and linear._kernels_take(flat)
            and cabi_x.mx_wgrad_serves(rows, hidden, width, format) and cabi_x.mx_wgrad_serves(rows, width, out_features, format))


def _plain_mlp(x, fc1_weight, fc2_weight, fc1_bias, fc2_bias, activation: str, format: str) -> torch.Tensor:
    """the forward of the node with nothing kept: the same kernel with the buffer absent where the node would run it, the same bytes"""
    u = F.linear(x, fc1_weight, fc1_bias)
    rows = u.reshape(-1, u.shape[-1])
    if _serves(x.reshape(-1, x.shape[-1]), rows, fc2_weight.shape[0], format):
        h = cabi_x.mx_act_forward(linear._unit_stride(rows), activation, format, keep=False)[0].view(u.shape)
    else:
        h = _torch_act(u, activation)
    return F.linear(h, fc2_weight, fc2_bias)


class _MLPMX(torch.autograd.Function):
    """``fc2(act(fc1(x)))`` as ONE node (:func:`mlp_mx`).  Kept for backward: ``x`` as the row blocks of a seed (one uint8 buffer; only while ``fc1_weight``
    requires grad), ``u`` as another (only while something other than ``fc2_bias`` requires grad) and the two weights.  On ``ctx``: ``seeds``
    (``glu._mx_seeds``; None where nothing is rounded), ``served`` (whether the kernels of fewbit_mxact.hip and ``mx_wgrad`` run).  Nothing of the shape
    of ``x``, ``u`` or ``h`` in a float dtype."""

    @staticmethod
    def forward(ctx, x, fc1_weight, fc2_weight, fc1_bias, fc2_bias, activation: str, format: str, generator):
        needs = ctx.needs_input_grad
        ctx.activation, ctx.format, ctx.input_shape, ctx.input_dtype = activation, format, tuple(x.shape), x.dtype
        ctx.autocast = linear._autocast_seen(x.device.type)
        keeps_x, keeps_u = needs[1], any(needs[:4])
        flat = x.detach().reshape(-1, x.shape[-1])
        u = F.linear(x, fc1_weight, fc1_bias)
        lead, width = u.shape[:-1], u.shape[-1]
        u = u.reshape(-1, width)
        rows, hidden = flat.shape
        out_features = fc2_weight.shape[0]
        ctx.flat_shape, ctx.width = (rows, hidden), width
        ctx.served = _serves(flat, u, out_features, format)
        ctx.seeds = None
        if keeps_u:
            on_device = linear._kernels_take(u)
            ctx.seeds = _mx_seeds(linear._sketch_seed(generator, u.device) if on_device else
                                  linear._draw_seed(generator if generator is None or generator.device.type == 'cpu' else None))
        x_kept = (_mx_keep(flat, ctx.seeds(0, 1), format), ) if keeps_x else ()
        if ctx.served:
            # (with nothing to keep: the same kernel with the buffer absent, the same bytes of h)
            h, state = cabi_x.mx_act_forward(linear._unit_stride(u), activation, format, ctx.seeds(1, 2) if keeps_u else 0, keep=keeps_u)
            u_kept = (state, ) if keeps_u else ()
        else:
            u_kept = (_mx_keep(u, ctx.seeds(1, 2), format), ) if keeps_u else ()
            h = _torch_act(u, activation)
        ctx.layout = (len(x_kept), len(u_kept))
        ctx.save_for_backward(*x_kept, *u_kept, fc1_weight, fc2_weight)
        return F.linear(h.view(*lead, width), fc2_weight, fc2_bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        with linear._autocast_as(ctx.autocast):
            return _MLPMX._backward(ctx, linear._dense_rows(grad_output))

    @staticmethod
    def _backward(ctx, grad_output):
        saved = ctx.saved_tensors                           # read once: a non-re-entrant checkpoint unpacks a saved tensor one time only
        of_x, of_u = ctx.layout
        x_kept, u_kept, (fc1_weight, fc2_weight) = saved[:of_x], saved[of_x:of_x + of_u], saved[of_x + of_u:]
        needs, format, seeds = ctx.needs_input_grad, ctx.format, ctx.seeds
        (rows, hidden), width = ctx.flat_shape, ctx.width
        out_features = fc2_weight.shape[0]
        G = grad_output.reshape(-1, grad_output.shape[-1])
        if ctx.served and G.dtype not in DTYPES:
            G = G.float()
        # du as a tensor (dx and the bias sum read it), du as fp8 cells (d fc1_weight), h^ as cells (d fc2_weight)
        want = (needs[0] or needs[3], needs[1], needs[2])
        gh = G @ fc2_weight if any(want[:2]) else None
        du = by_fc1 = by_fc2 = None
        if ctx.served and any(want):
            if gh is None:
                gh = torch.zeros((rows, width), dtype=G.dtype, device=G.device)      # (only d fc2_weight is wanted: h^ does not depend on gh)
            elif gh.dtype not in DTYPES:
                gh = gh.float()
            du, du_cells, product_cells = cabi_x.mx_act_backward(gh, u_kept[0], ctx.activation, format, seeds(2, 4), want)
            to = lambda weight: weight.dtype if weight.dtype in DTYPES else torch.float32
            if needs[1]:
                by_fc1 = cabi_x.mx_wgrad(du_cells, x_kept[0], rows, hidden, width, format, to(fc1_weight))
            if needs[2]:
                # (the one stand-alone pack of backward: grad_output)
                by_fc2 = cabi_x.mx_wgrad(_mx_keep(G, seeds(4, 5), 'fp8', 'grad'), product_cells, rows, width, out_features, format, to(fc2_weight))
        elif any(want):
            # the composed route: the same mathematics from mx_pack / mx_unpack (or their host forms) and torch's formulas, with the EXACT gradients --
            # nothing is rounded to fp8 here
            work = G.dtype if gh is None else gh.dtype
            u_hat = _mx_decoded(u_kept[0], (rows, width), format, work)
            nan = torch.full((), float('nan'), dtype=work, device=G.device)
            poisoned = torch.isnan(u_hat)
            if want[0] or want[1]:
                du = torch.where(poisoned, nan, gh * _slope(u_hat, ctx.activation))
            if needs[1]:
                by_fc1 = du.T @ _mx_decoded(x_kept[0], (rows, hidden), format, work)
            if needs[2]:
                product = torch.where(poisoned, nan, _torch_act(u_hat, ctx.activation))
                by_fc2 = G.T @ _mx_decoded(_mx_keep(product, seeds(3, 4), format), (rows, width), format, G.dtype)
        grads = [None] * 8
        if needs[0]:
            grads[0] = (du @ fc1_weight).view(ctx.input_shape).to(ctx.input_dtype)
        if needs[1]:
            grads[1] = by_fc1.to(fc1_weight.dtype)
        if needs[2]:
            grads[2] = by_fc2.to(fc2_weight.dtype)
        if needs[3]:
            grads[3] = du.sum(dim=0)
        if needs[4]:
            grads[4] = G.sum(dim=0)
        return tuple(grads)


def mlp_mx(x: torch.Tensor, fc1_weight: torch.Tensor, fc2_weight: torch.Tensor, fc1_bias: Optional[torch.Tensor] = None,
           fc2_bias: Optional[torch.Tensor] = None, activation: str = 'gelu', format: str = 'fp6', generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """``F.linear(act(F.linear(x, fc1_weight, fc1_bias)), fc2_weight, fc2_bias)``, the feed-forward block of the LayerNorm models, as ONE node that
    keeps ``x`` and ``u = fc1(x)`` as MXFP4 (``format='fp4'``) or MXFP6 (``'fp6'``) cells down their columns and nothing of ``h = act(u)``: per token
    of 768 -> 3072 in bf16, 2040 (fp4) or 3000 (fp6) bytes where torch keeps ``x``, ``u`` and ``h`` (13824) and ``MXLinear`` -> ``GELU(bits=3)`` ->
    ``MXLinear`` keeps 3192 at fp4.  ``activation``: ``'gelu'`` (the erf form), ``'gelu_tanh'`` (GPT-2's ``gelu_new``), ``'relu'`` (OPT), ``'silu'``.

    * Forward: ``x^ = mx_pack(x)``, torch's ``fc1``, ONE launch (``cabi_x.mx_act_forward``) that writes ``h`` -- ``act`` in fp32, rounded once -- and ``u``
      as cells, torch's ``fc2``.
    * Backward: ``gh = G @ fc2_weight``; ONE launch (``cabi_x.mx_act_backward``) decodes ``u^``, writes ``du = gh * act'(u^)`` and, while it holds
      them, the same ``du`` as fp8 cells and ``h^ = act(u^)`` as cells only; then ``d fc1_weight = mx_wgrad(du cells, x^)`` and
      ``d fc2_weight = mx_wgrad(mx_pack(G, 'fp8'), h^ cells)``, both on the scaled matrix instruction, nothing decoded.  ``dx = du @ fc1_weight`` and
      the bias gradients (column sums) use the unrounded ``du`` and ``G``.
    * What is rounded twice: ``h^`` is rebuilt from the rounded ``u^`` and then rounded into cells; ``du`` is formed from ``u^`` and then rounded to fp8
      cells for the weight gradient.  Every rounding is unbiased given its input, but ``act`` is not linear: ``du`` and ``d fc2_weight`` carry the bias
      of second order in the step that :func:`gated_mlp_quantized` states for the integer form.
    * Seeds: ONE draw from ``linear._sketch_seed`` per call (none where only ``fc2_bias`` requires grad); the five rounded tensors (``MLP_MX_SEEDS``)
      take it plus 0 .. 4, so no two tensors share a seed.  While the stream is being captured the draw is a device word and so are the five.
    * Served on the kernels: fp16 / bf16 GPU tensors whose three widths are multiples of 32 (``cabi_x.mx_wgrad_serves``) while
      ``linear.use_native_sketch()`` is on.  Every other call -- host tensors, fp32, float64, other widths -- composes the same mathematics from
      ``mx_pack`` / ``mx_unpack`` or their host forms and torch's formulas with the EXACT gradients (no fp8 rounding), as :func:`gated_mlp_mx` does.
    * Only what a requested gradient can need is kept or written.  Grad mode off, or nothing that requires grad: the plain forward -- no seed is
      drawn, nothing is kept, the same bytes.
    * Backward runs under the autocast state the forward saw; not differentiable twice; inside ``torch.utils.checkpoint`` ``generator`` must be a
      default one (``None`` included)."""
    _check(activation, format)
    tensors = (x, fc1_weight, fc2_weight, fc1_bias, fc2_bias)
    if not kept.trains(*tensors) or x.numel() == 0:
        if x.numel() == 0:
            return F.linear(_torch_act(F.linear(x, fc1_weight, fc1_bias), activation), fc2_weight, fc2_bias)
        return _plain_mlp(*(None if t is None else t.detach() for t in tensors), activation, format)
    return _MLPMX.apply(*tensors, activation, format, generator)


class MXMLP(torch.nn.Module):
    r"""``fc2(act(fc1(x)))`` as ONE node that keeps ``x`` and ``fc1(x)`` as MXFP4 / MXFP6 cells and forms both weight gradients on the scaled matrix
    instruction of gfx950 (:func:`mlp_mx`).  ``fc1`` and ``fc2`` are plain ``nn.Linear`` layers.  Parameters: ``in_features``, ``intermediate``,
    ``out_features`` (default ``in_features``), ``bias`` (default True), ``activation`` (``'gelu'``, ``'gelu_tanh'``, ``'relu'`` or ``'silu'``), ``format``
    (``'fp4'`` or ``'fp6'``, the default), ``generator``, ``device``, ``dtype``.  In ``eval()`` mode gradients that are asked for are torch's exact ones.

        >>> block.mlp = fewbit.MXMLP.from_linears(block.mlp.fc1, block.mlp.fc2, activation='gelu', format='fp6')
    """

    def __init__(self, in_features: int, intermediate: int, out_features: Optional[int] = None, bias: bool = True, activation: str = 'gelu',
                 format: str = 'fp6', generator: Optional[torch.Generator] = None, device=None, dtype=None) -> None:
        _check(activation, format)
        super().__init__()
        self.activation, self.format, self.generator = activation, format, generator
        self.fc1 = torch.nn.Linear(in_features, intermediate, bias, device, dtype)
        self.fc2 = torch.nn.Linear(intermediate, in_features if out_features is None else out_features, bias, device, dtype)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        fc1, fc2 = self.fc1, self.fc2
        if kept.exact_in_eval(self, x, *self.parameters()):
            return fc2(_torch_act(fc1(x), self.activation))
        return mlp_mx(x, fc1.weight, fc2.weight, fc1.bias, fc2.bias, self.activation, self.format, self.generator)

    def extra_repr(self) -> str:
        return f'activation={self.activation!r}, format={self.format!r}'

    @classmethod
    def from_linears(cls, fc1: torch.nn.Linear, fc2: torch.nn.Linear, activation: str = 'gelu', format: str = 'fp6',
                     generator: Optional[torch.Generator] = None) -> 'MXMLP':
        """An ``MXMLP`` that SHARES two built ``nn.Linear`` layers (``fc2`` takes what ``fc1`` gives)"""
        if not isinstance(fc1, torch.nn.Linear) or not isinstance(fc2, torch.nn.Linear) or fc2.in_features != fc1.out_features:
            raise ValueError('fc1 and fc2 should be nn.Linear layers with fc2.in_features == fc1.out_features.')
        new = cls(1, 1, activation=activation, format=format, generator=generator, device='meta')
        new.fc1, new.fc2 = fc1, fc2
        return new.train(fc1.training)
