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

``linear_cross_entropy`` goes one step further back: the LM head and the loss as ONE node, so that the logits themselves -- the largest tensor a
swapped model still allocates, 4.2 GB at 16384 tokens x 128256 classes in bf16, and as much again for their gradient -- exist one chunk of rows at
a time.  That is possible for ``'mean'`` and ``'sum'`` because the gradient arriving at a row's loss is known in the forward pass, up to the scalar
``grad_output``: ``1 / count`` or ``1``.  Per chunk the node runs the head's GEMM into one reused buffer, turns the chunk into its own gradient in
place while taking its loss (``cabi_x.cross_entropy_step``: ONE launch that reads every logit from HBM once and writes it once; the row waits in
LDS between the reduction and the gradient -- up to 81856 16-bit or 40928 fp32 classes; a longer row takes the two launches above), and feeds that gradient straight into the GEMMs of ``dx`` and ``dW``.  Backward multiplies the three
finished gradients by ``grad_output``.  The GEMMs are torch's (hipBLASLt); the logits still leave the chip once per chunk.
"""
from typing import Optional

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import linear

__all__ = ('cross_entropy', 'CrossEntropyLoss', 'linear_cross_entropy', 'LinearCrossEntropyLoss', 'default_chunk_rows')

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


# ---- the LM head and the loss as one node: the logits exist one chunk of rows at a time ---------------------------------------------------------------
def default_chunk_rows(rows: int, hidden: int, classes: int) -> int:
    """The rows of a chunk where none are asked for: the smallest power of two at or above ``rows * hidden / classes`` -- a chunk of logits about the
    size of the hidden states -- but at least 4096 and at most ``rows``.  The floor is measured (EXPERIMENTS.md 8.30): at 16384 tokens chunks of 1024
    rows made the step 1.5 to 2.0 times as slow as whole logits in bf16, chunks of 4096 rows 1.09 to 1.28 times."""
    want = max(1, -(-rows * hidden // classes))
    return max(1, min(rows, max(4096, 1 << (want - 1).bit_length())))


class _LinearCrossEntropy(torch.autograd.Function):
    """Computes the loss AND the three gradients forward, chunk by chunk; saves the gradients, which backward scales by ``grad_output``."""

    @staticmethod
    def forward(ctx, x, weight, target, bias, ignore_index: int, reduction: str, chunk_rows: int, accumulate_dtype, out_dtype):
        from . import cabi_x
        rows, classes = x.shape[0], weight.shape[0]
        want_x, want_w, _, want_b = ctx.needs_input_grad[:4]
        want_b = want_b and bias is not None
        with torch.autocast('cuda', enabled=False):
            if reduction == 'mean':
                scale = (target != ignore_index).sum().to(torch.float32).reciprocal().reshape(1)
            else:
                scale = torch.ones(1, dtype=torch.float32, device=x.device)
            logits = torch.empty((min(chunk_rows, rows), classes), dtype=x.dtype, device=x.device)
            lse, loss = torch.empty(rows, dtype=torch.float32, device=x.device), torch.empty(rows, dtype=torch.float32, device=x.device)
            dx = torch.empty_like(x) if want_x else None
            # (written by the first chunk, added to by the others: nothing is cleared, so a captured graph holds kernels and GEMMs only)
            dw = torch.empty(weight.shape, dtype=accumulate_dtype, device=x.device) if want_w else None
            db = torch.empty(classes, dtype=accumulate_dtype, device=x.device) if want_b else None
            for start in range(0, rows, chunk_rows):
                stop = min(start + chunk_rows, rows)
                x_c, d_c = x[start:stop], logits[:stop - start]
                if bias is None:
                    torch.mm(x_c, weight.t(), out=d_c)
                else:
                    torch.addmm(bias, x_c, weight.t(), out=d_c)
                cabi_x.cross_entropy_step(d_c, target[start:stop], scale, ignore_index, lse[start:stop], loss[start:stop])      # (d_c: now the gradient)
                if want_x:
                    torch.mm(d_c, weight, out=dx[start:stop])
                if want_w and dw.dtype == x.dtype:
                    torch.mm(d_c.t(), x_c, out=dw) if start == 0 else dw.addmm_(d_c.t(), x_c)
                elif want_w:                                                         # (the chunk's product in the operands' dtype, the running sum wider)
                    dw.copy_(torch.mm(d_c.t(), x_c)) if start == 0 else dw.add_(torch.mm(d_c.t(), x_c))
                if want_b:
                    torch.sum(d_c, 0, dtype=accumulate_dtype, out=db) if start == 0 else db.add_(d_c.sum(0, dtype=accumulate_dtype))
            out = loss.sum()
            if reduction == 'mean':
                out = out * scale[0]
            kept = [None if g is None else g.to(like.dtype) for g, like in ((dx, x), (dw, weight), (db, bias))]
        ctx.save_for_backward(*(g for g in kept if g is not None))
        ctx.have, ctx.spent = tuple(g is not None for g in kept), False
        return out.to(out_dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        if ctx.spent:
            raise RuntimeError('linear_cross_entropy: the gradients were computed forward and scaled by grad_output in the first backward(); '
                               'a second backward through this node is not possible')
        ctx.spent = True
        kept, g = iter(ctx.saved_tensors), grad_output.to(torch.float32)
        dx, dw, db = (next(kept).mul_(g) if have else None for have in ctx.have)
        return dx, dw, None, db, None, None, None, None, None


def _linear_kernel_applies(input, weight, target, bias, reduction: str) -> bool:
    if not (linear.use_native_sketch() and reduction in ('mean', 'sum') and torch.is_grad_enabled()):
        return False
    tensors = (input, weight) + (() if bias is None else (bias, ))
    if not all(isinstance(t, torch.Tensor) for t in tensors + (target, )):
        return False
    if any(t.device != input.device or t.dtype != input.dtype for t in tensors) or input.device.type != 'cuda' or input.dtype not in _KERNEL_DTYPES:
        return False
    if target.dtype != torch.int64 or target.device != input.device or not any(t.requires_grad for t in tensors):
        return False
    if weight.dim() != 2 or input.dim() < 1 or input.shape[-1] != weight.shape[1] or (bias is not None and bias.shape != weight.shape[:1]):
        return False
    return min(weight.shape) >= 1 and input.numel() >= 1 and target.numel() * weight.shape[1] == input.numel()


def linear_cross_entropy(input: torch.Tensor, weight: torch.Tensor, target: torch.Tensor, bias: Optional[torch.Tensor] = None, *, ignore_index: int = -100,
                         reduction: str = 'mean', chunk_rows: Optional[int] = None, accumulate_dtype: Optional[torch.dtype] = None,
                         out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``cross_entropy(F.linear(input, weight, bias), target)`` -- an LM head and its loss -- as one node that never holds the logits or their gradient
    whole (module docstring): ``F.cross_entropy(F.linear(input, weight, bias).float(), target, ...)`` rounded once to ``out_dtype`` (default: fp32 under
    ``torch.autocast`` on the GPU, else the input's dtype).

    ``input``: ``(..., H)``, taken as ``(N, H)``; ``weight``: ``(V, H)``; ``target``: int64 of ``N`` elements in any shape; ``bias``: ``(V,)``.

    ``chunk_rows``: the rows whose logits exist at a time, in one reused ``(chunk_rows, V)`` buffer (default: :func:`default_chunk_rows`).  The
    allocator's peak is about that buffer plus the gradients themselves, instead of one to two ``(N, V)`` tensors.

    ``accumulate_dtype``: the dtype in which ``dW`` and ``db`` run from chunk to chunk (default: the weight's; ``torch.float32`` costs a ``(V, H)``
    fp32 tensor and the chunk's product beside it); they are cast once at the end.

    The gradients are COMPUTED IN THE FORWARD PASS, for whichever of ``input``, ``weight`` and ``bias`` require one; ``backward()`` multiplies them by
    ``grad_output`` in place, and a second ``backward()`` through the node raises (also with ``retain_graph=True``).  Nothing is read back and the
    number of chunks depends on the shapes only: the call can be captured into a hipGraph.

    The kernel path needs GPU tensors of one dtype among fp32 / fp16 / bf16 (under ``torch.autocast`` they are cast to its dtype first, as
    ``F.linear`` casts them), ``reduction`` ``'mean'`` or ``'sum'``, grad mode on and something that requires grad, while
    ``linear.use_native_sketch()`` is on.  Everything else -- ``'none'``, host tensors, float64, ``no_grad`` -- is
    :func:`cross_entropy` of ``F.linear(input, weight, bias)`` with the rows flattened, and ignores ``chunk_rows`` and ``accumulate_dtype``."""
    if reduction not in ('none', 'mean', 'sum'):
        raise ValueError(f'{reduction} is not a valid value for reduction')
    autocast = isinstance(input, torch.Tensor) and input.device.type == 'cuda' and torch.is_autocast_enabled('cuda')
    if autocast:
        to = torch.get_autocast_dtype('cuda')
        input, weight, bias = input.to(to), weight.to(to), None if bias is None else bias.to(to)
    if not _linear_kernel_applies(input, weight, target, bias, reduction):
        logits = F.linear(input, weight, bias)
        out = cross_entropy(logits.reshape(-1, logits.shape[-1]), target.reshape(-1), ignore_index=ignore_index, reduction=reduction, out_dtype=out_dtype)
        return out.reshape(target.shape) if reduction == 'none' else out
    x, t = input.reshape(-1, input.shape[-1]), target.reshape(-1).contiguous()
    if chunk_rows is None:
        chunk_rows = default_chunk_rows(x.shape[0], x.shape[1], weight.shape[0])
    if int(chunk_rows) < 1:
        raise ValueError(f'chunk_rows = {chunk_rows} must be at least 1')
    if out_dtype is None:
        out_dtype = torch.float32 if autocast else input.dtype
    return _LinearCrossEntropy.apply(x, weight, t, bias, int(ignore_index), reduction, int(chunk_rows), accumulate_dtype or weight.dtype, out_dtype)


class LinearCrossEntropyLoss(torch.nn.Module):
    """:func:`linear_cross_entropy` as a module: ``loss(hidden, head.weight, target, head.bias)`` in place of ``CrossEntropyLoss()(head(hidden), target)``,
    with the logits held one chunk of rows at a time.  It owns no parameters: the head's weight is passed in, tied or not."""

    def __init__(self, ignore_index: int = -100, reduction: str = 'mean', chunk_rows: Optional[int] = None, accumulate_dtype: Optional[torch.dtype] = None,
                 out_dtype: Optional[torch.dtype] = None):
        super().__init__()
        self.ignore_index, self.reduction, self.chunk_rows, self.accumulate_dtype, self.out_dtype = ignore_index, reduction, chunk_rows, accumulate_dtype, out_dtype

    def forward(self, input: torch.Tensor, weight: torch.Tensor, target: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        return linear_cross_entropy(input, weight, target, bias, ignore_index=self.ignore_index, reduction=self.reduction, chunk_rows=self.chunk_rows,
                                    accumulate_dtype=self.accumulate_dtype, out_dtype=self.out_dtype)

    def extra_repr(self) -> str:
        return (f'ignore_index={self.ignore_index}, reduction={self.reduction!r}, chunk_rows={self.chunk_rows}, accumulate_dtype={self.accumulate_dtype}, '
                f'out_dtype={self.out_dtype}')
