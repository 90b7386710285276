"""Dropout that saves nothing for backward: the mask is a function of a 64-bit seed.

``torch.nn.Dropout`` keeps one ``bool`` -- one byte -- per element for backward: for a bf16 model half as much as the activation itself.
Here the mask of a call is a pure function of (seed, threshold, element index) that host and kernel evaluate alike (include/fewbit_hipx.h,
"the mask of a seed"; ``cabi_x.dropout_keep`` is the host evaluation), so the autograd node keeps ONE integer and no tensor, and backward
regenerates the mask from the seed with the kernel that made it in forward (``fewbit_amd/csrc/fewbit_dropout.hip``, one launch each way).

* The drop probability is realized as ``T / 65536`` with ``T = round(p * 65536)`` (``cabi_x.dropout_threshold``; ``|p - T / 65536| <= 2^-17``)
  and the kept elements are scaled by ``float32(65536 / (65536 - T))``, so ``E[out] = input`` exactly.  ``T = 0`` (``p < 2^-17``) drops nothing.
* A dropped element is exactly ``+0`` whatever the input holds.  torch gives NaN for a dropped inf or NaN; here that element has no
  influence on the result.
* The seed comes from ``linear._sketch_seed``: one draw from the host generator per call, so ``torch.manual_seed`` reproduces a run -- and a
  model's other random streams move by one host draw per call relative to ``nn.Dropout``, which draws on the device.  While the stream is
  being captured into a hipGraph the seed is a device word fed by the per-device replay counter: every replay draws a fresh mask, and the
  recorded backward reads the same word as its forward.  (One eager call on the device precedes a capture, as for the randomized linears.)
* The kernel serves fp32 / fp16 / bf16 GPU tensors with at least one element while ``linear.use_native_sketch()`` is on.  Host tensors,
  float64 and ``use_native_sketch(False)`` take ``torch.nn.functional.dropout`` unchanged.
* Not differentiable twice (``once_differentiable``); ``torch.func.grad`` / ``torch.vmap`` refuse the node (it has no ``setup_context``).
* Inside training wrappers (tests/test_dropout_training.py, tests/test_gpu_dropout_training.py): under ``torch.autocast`` a 16-bit input stays
  16-bit and ``backward()`` may follow the block; under ``torch.utils.checkpoint`` in both modes the recomputation draws the forward's seed
  again, so output and gradients are the plain run's bit for bit -- PROVIDED the seed comes from a default generator (``generator=None``,
  ``torch.default_generator``, ``torch.cuda.default_generators[i]``): checkpoint saves and restores only those.  With any other generator
  the recomputation draws a SECOND seed: in non-reentrant mode the node keeps the forward's seed while the layers behind it receive
  activations recomputed under another mask; in reentrant mode every gradient belongs to another mask than the output.  Nothing raises.
* With grad mode off (``no_grad``, ``inference_mode``) a call still drops and builds no node; ``inplace=True`` then writes through the binding
  and returns the input object itself, as torch does -- a leaf that requires grad keeps requiring it.
"""
from typing import Optional

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import linear

__all__ = ('dropout', 'dropout_add', 'Dropout')

_KERNEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _check_p(p: float) -> None:
    if not 0.0 <= p <= 1.0:                                             # (NaN fails both comparisons)
        raise ValueError(f'dropout probability has to be between 0 and 1, but got {p}')


def _kernel_applies(input: torch.Tensor) -> bool:
    return linear.use_native_sketch() and input.device.type == 'cuda' and input.dtype in _KERNEL_DTYPES and input.numel() > 0


class _SeededDropout(torch.autograd.Function):
    """``[residual +] dropout(input)`` on the kernel.  Saves no tensor: ``ctx`` keeps the seed (an int; a device word while capturing) and p."""

    @staticmethod
    def forward(ctx, input, residual, p: float, inplace: bool, generator):
        from . import cabi_x
        ctx.seed, ctx.p = linear._sketch_seed(generator, input.device), p
        src = input if input.is_contiguous() else input.contiguous()
        addend = None if residual is None else residual.contiguous()
        if not inplace:
            return cabi_x.dropout_apply(src, ctx.seed, p, addend)
        ctx.mark_dirty(input)
        cabi_x.dropout_apply(src, ctx.seed, p, addend, out=src)
        if src is not input:
            input.copy_(src)
        return input

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        from . import cabi_x
        grad_input = None
        if ctx.needs_input_grad[0]:
            grad_input = cabi_x.dropout_apply(grad_output.contiguous(), ctx.seed, ctx.p)
        return grad_input, grad_output if ctx.needs_input_grad[1] else None, None, None, None


def dropout(input: torch.Tensor, p: float = 0.5, training: bool = True, inplace: bool = False,
            generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """``torch.nn.functional.dropout`` whose backward needs no mask: on the kernel path (module docstring) the node saves no tensor, the mask
    is regenerated from the call's seed.  ``generator``: where the seed is drawn from (default: the host default generator).  Not training,
    or a threshold of 0: the input itself -- no launch, no node, no seed drawn.  A non-contiguous input gives a contiguous output; with
    ``inplace=True`` the result is written into the input (with grad mode off the input object itself is returned).  A dropped element is +0
    even where the input is inf or NaN.  Inside ``torch.utils.checkpoint`` ``generator`` must be a default one (``None`` included): checkpoint
    restores only those, and the recomputation must draw the forward's seed again (module docstring)."""
    _check_p(p)
    if not training or p == 0.0:
        return input
    if not _kernel_applies(input):
        return F.dropout(input, p, True, inplace)
    from . import cabi_x
    if cabi_x.dropout_threshold(p) == 0:
        return input
    if inplace and input.requires_grad and input.is_leaf and torch.is_grad_enabled():         # (before anything is written, as in torch)
        raise RuntimeError('a leaf Variable that requires grad is being used in an in-place operation.')
    if inplace and not torch.is_grad_enabled():
        # no node to build: written through the binding, and the caller gets its own tensor back (``Function.apply`` with grad mode off
        # returns another tensor object that no longer requires grad, which ``x = drop(x)`` would silently keep)
        src = input if input.is_contiguous() else input.contiguous()
        cabi_x.dropout_apply(src, linear._sketch_seed(generator, input.device), float(p), out=src)
        if src is input:
            torch.autograd.graph.increment_version(input)             # (the write went through a pointer: autograd is told, as mark_dirty tells it)
        else:
            input.copy_(src)
        return input
    return _SeededDropout.apply(input, None, float(p), inplace, generator)


def dropout_add(input: torch.Tensor, residual: torch.Tensor, p: float = 0.5, training: bool = True,
                generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """``residual + dropout(input)``, a transformer sublayer's ending, in one launch on the kernel path: the sum is made in fp32 and rounded once
    (a dropped element gives the residual's bits).  The gradient of ``residual`` is ``grad_output`` itself, that of ``input`` one kernel call.
    Unequal shapes, dtypes or devices and everything off the kernel path compute ``residual + dropout(input, ...)``."""
    _check_p(p)
    if not training or p == 0.0:
        return residual + input
    if not (_kernel_applies(input) and residual.shape == input.shape and residual.dtype == input.dtype and residual.device == input.device):
        return residual + dropout(input, p, True, False, generator)
    from . import cabi_x
    if cabi_x.dropout_threshold(p) == 0:
        return residual + input
    return _SeededDropout.apply(input, residual, float(p), False, generator)


class Dropout(torch.nn.Dropout):
    """:class:`torch.nn.Dropout` that keeps nothing for backward (:func:`dropout`): one integer per call instead of one byte per element.
    ``m.eval()`` turns it off; ``isinstance(m, torch.nn.Dropout)`` holds.  Swap it into a model with::

        fewbit.map_module(model, lambda m, path: fewbit.Dropout(m.p, m.inplace) if type(m) is torch.nn.Dropout else m)

    The seed of a call is a draw from the host generator (``generator``, default: torch's default one), so ``torch.manual_seed`` reproduces a
    run, and a model's other random streams move by one host draw per call relative to ``nn.Dropout``.  Inside ``torch.utils.checkpoint`` the
    generator must be a default one (``None``, ``torch.default_generator``, ``torch.cuda.default_generators[i]``): checkpoint saves and
    restores only those, so a generator of the caller's own draws a second seed in the recomputation and the gradients no longer belong to
    the mask of the output (module docstring)."""

    def __init__(self, p: float = 0.5, inplace: bool = False, generator: Optional[torch.Generator] = None):
        super().__init__(p, inplace)
        self.generator = generator

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        return dropout(input, self.p, self.training, self.inplace, self.generator)
