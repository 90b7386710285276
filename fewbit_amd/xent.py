"""Cross entropy that keeps the logits as given and one float per row.

``torch.nn.functional.cross_entropy`` is ``log_softmax`` followed by ``nll_loss``, and its node keeps the whole ``log_softmax`` output for
backward -- in fp32 wherever the logits are cast first, as the Hugging Face losses do (``logits.float()``) and as ``torch.autocast`` does:
twice the bytes of bf16 logits, beside an fp32 copy of the logits, an fp32 gradient and its cast back.  The arithmetic needs none of it: one
read of the logits forward, one read and one write backward, and the log-sum-exp of every row in between.

Here the node of a call saves the ``input`` tensor ITSELF (no copy, no cast -- the LM head's output, which is alive anyway), the targets and
one fp32 number per row (include/fewbit_hipx.h, "The loss of a row"; ``fewbit_amd/csrc/fewbit_xent.hip``, one launch each way).

* The kernel serves GPU tensors of fp32 / fp16 / bf16 that are 1-D ``(C,)`` or 2-D ``(N, C)`` with unit stride along the classes -- a
  row-sliced view (``logits[:, :-1]`` flattened, ``logits[::2]``) is taken as it is, through its row stride -- with int64 class indices of
  shape ``(N,)`` (0-d for a 1-D input), ``weight=None`` and ``label_smoothing=0``, while ``linear.use_native_sketch()`` is on.  Everything
  else -- host tensors, float64, class weights, label smoothing, probability targets, ``(N, C, d1, ...)`` inputs -- calls
  ``F.cross_entropy`` unchanged (and ignores the two extra keywords).
* Arithmetic is fp32 whatever the dtypes, and the loss is rounded ONCE to ``out_dtype``: by default fp32 while
  ``torch.is_autocast_enabled('cuda')`` -- torch's own result there -- and the input's dtype otherwise.
  ``cross_entropy(logits, t, out_dtype=torch.float32)`` replaces ``F.cross_entropy(logits.float(), t)``.
* ``'sum'`` and ``'mean'`` are torch reductions of the fp32 per-row losses; the mean divides by ``(target != ignore_index).sum()`` on the
  device, so a mean over no row is NaN as in torch, and nothing is read back: the call can be captured into a hipGraph.
* A target outside ``[0, C)`` that is not ``ignore_index`` gives a NaN loss and a NaN gradient row; torch asserts on the device.
* The gradient of a row-sliced input is a contiguous tensor; where its rows start at other offsets from a 16-byte boundary than the input's, backward
  stores element by element instead of by 16-byte pieces: the same values, slower (not measured).  In place the offsets always agree.
* Not differentiable twice (``once_differentiable``).
* With grad mode off, or an input that needs no gradient: one forward launch, no node, nothing saved.
"""
from typing import Optional

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import linear

__all__ = ('cross_entropy', 'CrossEntropyLoss')

_KERNEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _kernel_applies(input: torch.Tensor, target: torch.Tensor, weight, label_smoothing: float) -> bool:
    if not (linear.use_native_sketch() and weight is None and label_smoothing == 0.0):
        return False
    if not (isinstance(input, torch.Tensor) and isinstance(target, torch.Tensor)):
        return False
    if input.device.type != 'cuda' or input.dtype not in _KERNEL_DTYPES or target.dtype != torch.int64 or target.device != input.device:
        return False
    if input.dim() == 1:
        return target.dim() == 0 and input.shape[0] >= 1 and (input.shape[0] == 1 or input.stride(0) == 1)
    if input.dim() != 2 or target.dim() != 1 or target.shape[0] != input.shape[0]:
        return False
    rows, width = input.shape
    return rows >= 1 and width >= 1 and (width == 1 or input.stride(1) == 1) and (rows == 1 or input.stride(0) >= width)


def _rows(input: torch.Tensor) -> torch.Tensor:
    return input if input.dim() == 2 else input.unsqueeze(0)


def _reduced(input: torch.Tensor, target: torch.Tensor, ignore_index: int, reduction: str, out_dtype: torch.dtype, want_node: bool):
    """the forward launch and the reduction -> (loss, targets as a vector, lse, 1 / count or None)"""
    from . import cabi_x
    t = target.reshape(-1).contiguous()
    lse, loss = cabi_x.cross_entropy_forward(_rows(input), t, ignore_index)
    scale = None
    if reduction == 'none':
        out = loss.reshape(target.shape)
    elif reduction == 'sum':
        out = loss.sum()
    else:
        count = (t != ignore_index).sum().to(torch.float32)
        out = loss.sum() / count
        if want_node:
            scale = count.reciprocal().reshape(1)
    return out.to(out_dtype), t, lse, scale


class _CrossEntropy(torch.autograd.Function):
    """Saves the input itself, the targets, the fp32 log-sum-exp of every row and, for 'mean', the one-element ``1 / count``."""

    @staticmethod
    def forward(ctx, input, target, ignore_index: int, reduction: str, out_dtype, inplace: bool):
        out, t, lse, scale = _reduced(input, target, ignore_index, reduction, out_dtype, True)
        ctx.save_for_backward(input, t, lse, *(() if scale is None else (scale, )))
        ctx.ignore_index, ctx.reduction, ctx.inplace, ctx.spent = ignore_index, reduction, inplace, False
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        from . import cabi_x
        if ctx.spent:
            raise RuntimeError('cross_entropy(inplace_backward=True): the logits were overwritten by the gradient in the first backward(); '
                               'a second backward through this node is not possible')
        input, t, lse, *scale = ctx.saved_tensors
        grow = grad_output.to(torch.float32)
        if ctx.reduction == 'mean':
            grow = grow * scale[0]
        grow = grow.reshape(-1).contiguous()                     # (one element for 'sum' / 'mean': the same for every row; one per row for 'none')
        x = _rows(input)
        if not ctx.inplace:
            return cabi_x.cross_entropy_backward(x, t, lse, grow, ctx.ignore_index).reshape(input.shape), None, None, None, None, None
        ctx.spent = True
        cabi_x.cross_entropy_backward(x, t, lse, grow, ctx.ignore_index, out=x)
        torch.autograd.graph.increment_version(input)            # (the write went through a pointer: whoever else saved the logits is told)
        return input.detach(), None, None, None, None, None


def cross_entropy(input: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None, size_average=None, ignore_index: int = -100,
                  reduce=None, reduction: str = 'mean', label_smoothing: float = 0.0, *, out_dtype: Optional[torch.dtype] = None,
                  inplace_backward: bool = False) -> torch.Tensor:
    """``torch.nn.functional.cross_entropy`` whose node keeps the logits as given and one float per row (module docstring): on the kernel path
    nothing of the size of the logits is allocated forward, and backward allocates the gradient only.

    ``out_dtype``: the dtype of the result (default: fp32 under ``torch.autocast`` on the GPU, else the input's); the arithmetic is fp32 and
    the value is rounded once, so ``out_dtype=torch.float32`` gives what ``F.cross_entropy(input.float(), target)`` gives, without the copy.

    ``inplace_backward=True`` writes the gradient over the saved logits and returns that tensor as the gradient, so backward allocates
    nothing at all.  THE LOGITS ARE GONE AFTER ``backward()``: ``input`` then holds its own gradient, whoever else reads it afterwards reads
    the gradient, and a second ``backward()`` through the node raises (also with ``retain_graph=True``).  Where ``input`` is a leaf that requires
    grad, ``input.grad`` is then the input's OWN memory: ``input`` and ``input.grad`` are one buffer, and an optimizer step on it would update the
    gradient it reads.  Default: off.

    Off the kernel path (host tensors, float64, ``weight``, ``label_smoothing``, probability targets, more than two dimensions,
    ``linear.use_native_sketch(False)``) the call is ``F.cross_entropy`` with the same arguments; the two extra keywords are ignored."""
    if not _kernel_applies(input, target, weight, label_smoothing):
        return F.cross_entropy(input, target, weight, size_average, ignore_index, reduce, reduction, label_smoothing)
    if size_average is not None or reduce is not None:
        reduction = torch.nn._reduction.legacy_get_string(size_average, reduce)
    if reduction not in ('none', 'mean', 'sum'):
        raise ValueError(f'{reduction} is not a valid value for reduction')
    if out_dtype is None:
        out_dtype = torch.float32 if torch.is_autocast_enabled('cuda') else input.dtype
    if not (torch.is_grad_enabled() and input.requires_grad):
        return _reduced(input, target, int(ignore_index), reduction, out_dtype, False)[0]
    return _CrossEntropy.apply(input, target, int(ignore_index), reduction, out_dtype, bool(inplace_backward))


class CrossEntropyLoss(torch.nn.CrossEntropyLoss):
    """:class:`torch.nn.CrossEntropyLoss` that keeps the logits as given and one float per row (:func:`cross_entropy`), with its two extra
    keywords ``out_dtype`` and ``inplace_backward`` (the logits are gone after ``backward()``, and a second backward raises).
    ``isinstance(m, torch.nn.CrossEntropyLoss)`` holds.  Swap it into a model with::

        fewbit.map_module(model, lambda m, path: fewbit.CrossEntropyLoss.from_loss(m) if type(m) is torch.nn.CrossEntropyLoss else m)

    A loss with class weights or label smoothing computes ``F.cross_entropy``."""

    def __init__(self, weight: Optional[torch.Tensor] = None, size_average=None, ignore_index: int = -100, reduce=None, reduction: str = 'mean',
                 label_smoothing: float = 0.0, *, out_dtype: Optional[torch.dtype] = None, inplace_backward: bool = False):
        super().__init__(weight, size_average, ignore_index, reduce, reduction, label_smoothing)
        self.out_dtype, self.inplace_backward = out_dtype, inplace_backward

    @classmethod
    def from_loss(cls, m: torch.nn.CrossEntropyLoss, *, out_dtype: Optional[torch.dtype] = None, inplace_backward: bool = False) -> 'CrossEntropyLoss':
        """The loss ``m`` with the same weight, ``ignore_index``, reduction and label smoothing"""
        return cls(m.weight, ignore_index=m.ignore_index, reduction=m.reduction, label_smoothing=m.label_smoothing, out_dtype=out_dtype,
                   inplace_backward=inplace_backward)

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return cross_entropy(input, target, weight=self.weight, ignore_index=self.ignore_index, reduction=self.reduction,
                             label_smoothing=self.label_smoothing, out_dtype=self.out_dtype, inplace_backward=self.inplace_backward)

    def extra_repr(self) -> str:
        return f'out_dtype={self.out_dtype}, inplace_backward={self.inplace_backward}'
