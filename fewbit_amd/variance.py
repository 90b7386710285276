"""Gradient-capture utilities and the variance estimator for randomized linear layers.

Counterpart of the reference's ``fewbit/functional/variance.py`` (``GradientStorage``, ``catch_gradients``) and
``fewbit/modules/variance.py`` (``VarianceEstimator``): same names and call shapes, own implementation.  For a linear
layer with input rows ``X`` (B x n) and output-gradient rows ``G`` (B x m) the exact weight gradient is ``G^T X``; the
module reports, per backward pass,

* ``corr     = (||X^T G||_F / (||X||_F ||G||_F))^2``
* ``var_sgd  = B/(B-1) * sum_b ||x_b||^2 ||g_b||^2 - ||X^T G||_F^2 / (B-1)``     (variance of the SGD estimate)
* ``var_rmm  = (||X||_F^2 ||G||_F^2 - ||X^T G||_F^2) / B_proj``                   (added by the random projection)

(definitions of fewbit/modules/variance.py:17-46; arXiv:2201.13195, section 3).

All three are functions of four numbers, ``gradient_moments``:

    sx = ||X||_F^2      sg = ||G||_F^2      sxg = sum_b ||x_b||^2 ||g_b||^2      cross = ||X^T G||_F^2
    corr = cross / (sx sg)      var_sgd = B/(B-1) sxg - cross/(B-1)      var_rmm = (sx sg - cross) / B_proj

On the GPU (fp32 / fp16 / bf16 operands, ``use_native_sketch()`` on) the first three come from ONE pass over X and G in their own dtypes
(``cabi_x.row_moments``: exact squares, fp64 sums in a fixed order) and the fourth from ONE GEMM in the operands' dtype with fp32
accumulation (``_cross_product``) followed by ``cabi_x.sum_squares`` -- no fp32 copies of the operands, nothing read back from the device,
so an estimator without a callback can be captured into a hipGraph together with its layer (after one eager step).  Operands of
different dtypes (autocast: fp32 input, bf16 gradient) are multiplied in the narrower one, the precision the layer's own exact
weight-gradient GEMM has there; fp16 with bf16 multiplies in bf16.  ``sx``, ``sg`` and ``sxg`` are always those of the operands as they are.
"""
from typing import Callable, Optional

import torch

from . import linear as _linear
from .linear import projection_dim

__all__ = ('GradientStorage', 'catch_gradients', 'VarianceEstimator', 'estimate_correlation', 'estimate_variance_sgd',
           'estimate_variance_rmm', 'gradient_moments', 'variance_path')


class GradientStorage:
    """Keeps a copy of a module's last input and of the gradient that reached its output."""

    def __init__(self):
        self.input = None
        self.grad_output = None

    def forward(self, input: torch.Tensor) -> None:
        self.input = input.detach().clone()

    def backward(self, grad_output: torch.Tensor) -> None:
        self.grad_output = grad_output.detach().clone()
        self.postprocess()

    def postprocess(self) -> None:
        """Hook for subclasses: called once both tensors of a step are in."""


class _Catch(torch.autograd.Function):

    @staticmethod
    def forward(ctx, input: torch.Tensor, storage: GradientStorage) -> torch.Tensor:
        ctx.storage = storage
        return input.view_as(input)

    @staticmethod
    def backward(ctx, grad_output: torch.Tensor):
        ctx.storage.backward(grad_output)
        return grad_output, None


def catch_gradients(input: torch.Tensor, storage: GradientStorage) -> torch.Tensor:
    """Identity whose backward hands the passing gradient to ``storage.backward``."""
    return _Catch.apply(input, storage)


class _CatchPair(torch.autograd.Function):
    """``catch_gradients`` for ONE call of a module that may be called several times before a backward: the copy of the call's input and its
    two row counts travel in the node (the copy as a saved tensor, so a checkpointed region releases it and recomputes it), and the storage
    receives the complete pair -- input, ``bs``, ``bs_proj``, then ``backward(grad_output)`` -- when the gradient of THIS call arrives."""

    @staticmethod
    def forward(ctx, output: torch.Tensor, kept: torch.Tensor, storage: GradientStorage, bs: int, bs_proj: int) -> torch.Tensor:
        ctx.storage, ctx.bs, ctx.bs_proj = storage, bs, bs_proj
        ctx.save_for_backward(kept)
        return output.view_as(output)

    @staticmethod
    def backward(ctx, grad_output: torch.Tensor):
        storage = ctx.storage
        (storage.input, ), storage.bs, storage.bs_proj = ctx.saved_tensors, ctx.bs, ctx.bs_proj
        storage.backward(grad_output)
        return grad_output, None, None, None, None


def estimate_correlation(input: torch.Tensor, output: torch.Tensor) -> torch.Tensor:
    cross = torch.linalg.norm(input.T @ output)
    return (cross / (torch.linalg.norm(input) * torch.linalg.norm(output)))**2


def estimate_variance_sgd(input: torch.Tensor, output: torch.Tensor, bs: Optional[int] = None) -> torch.Tensor:
    bs = bs or input.shape[0]
    rows = (input * input).sum(dim=1) @ (output * output).sum(dim=1)
    cross = torch.linalg.norm(input.T @ output)**2
    return rows * (bs / (bs - 1)) - cross / (bs - 1)


def estimate_variance_rmm(input: torch.Tensor, output: torch.Tensor, bs_proj: Optional[int] = None) -> torch.Tensor:
    bs_proj = bs_proj or input.shape[0]
    cross = torch.linalg.norm(input.T @ output)**2
    return (torch.linalg.norm(input)**2 * torch.linalg.norm(output)**2 - cross) / bs_proj


_KERNEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _native_moments_apply(x: torch.Tensor, g: torch.Tensor) -> bool:
    return (_linear.use_native_sketch() and x.device.type == 'cuda' and g.device == x.device and x.dtype in _KERNEL_DTYPES
            and g.dtype in _KERNEL_DTYPES and x.dim() == 2 and g.dim() == 2 and x.shape[0] == g.shape[0] and min(x.shape + g.shape) > 0)


def _cross_product(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """``G^T X`` as an fp32 matrix from ONE GEMM in the operands' dtype (fp32 accumulation).  Operands of different dtypes are rounded to
    the narrower one first (fp32 with a 16-bit dtype: that dtype; fp16 with bf16: bf16) -- the seam the tests count calls of."""
    if x.dtype != g.dtype:
        narrow = torch.bfloat16 if torch.bfloat16 in (x.dtype, g.dtype) else torch.float16
        x, g = x.to(narrow), g.to(narrow)
    if x.dtype == torch.float32:
        return torch.mm(g.T, x)
    return torch.mm(g.T, x, out_dtype=torch.float32)


def gradient_moments(input: torch.Tensor, grad_output: torch.Tensor) -> torch.Tensor:
    """``(sx, sg, sxg, cross)`` of a linear layer's input rows and output-gradient rows (leading dimensions are flattened) as a float64
    tensor of 4 elements on the operands' device (module docstring).  GPU operands take the gfx950 kernels and one GEMM; host tensors,
    float64 and ``use_native_sketch(False)`` take float64 PyTorch arithmetic.  Nothing is read back from the device."""
    x = input.reshape(-1, input.shape[-1])
    g = grad_output.reshape(-1, grad_output.shape[-1])
    if _native_moments_apply(x, g):
        from . import cabi_x
        out = torch.empty(4, dtype=torch.float64, device=x.device)
        workspace = torch.empty(cabi_x.moments_workspace_bytes(x.shape[0], x.shape[1], g.shape[1]), dtype=torch.uint8, device=x.device)
        cabi_x.row_moments(x, g, out=out[:3], workspace=workspace)
        cabi_x.sum_squares(_cross_product(x, g), out=out[3:], workspace=workspace)
        return out
    x, g = x.double(), g.double()
    xx, gg = (x * x).sum(dim=1), (g * g).sum(dim=1)
    product = x.T @ g
    return torch.stack((xx.sum(), gg.sum(), xx @ gg, (product * product).sum()))


def variance_path(input: torch.Tensor, grad_output: torch.Tensor) -> str:
    """Which code computes ``gradient_moments(input, grad_output)`` (what tools/variance_bench.py prints beside its times)."""
    x = input.reshape(-1, input.shape[-1])
    g = grad_output.reshape(-1, grad_output.shape[-1])
    if _native_moments_apply(x, g):
        gemm = str(x.dtype if x.dtype == g.dtype else (torch.bfloat16 if torch.bfloat16 in (x.dtype, g.dtype) else torch.float16)).replace('torch.', '')
        return (f'gfx950 kernels fewbit_hipx_row_moments (one pass over X and G, fp64 sums) + one {gemm} GEMM with fp32 accumulation + '
                'fewbit_hipx_sum_squares on its fp32 product')
    return 'float64 PyTorch arithmetic (fp64 copies of X and G, one fp64 GEMM)'


class _VarianceState(GradientStorage):

    def __init__(self, callback: Optional[Callable] = None):
        super().__init__()
        self.callback = callback
        self.step = 0
        self.variance = None
        self.bs = None
        self.bs_proj = None

    def postprocess(self) -> None:
        if self.input is None or self.grad_output is None:
            return
        sx, sg, sxg, cross = gradient_moments(self.input, self.grad_output).unbind(0)
        bs = self.bs or self.input.numel() // self.input.shape[-1]
        bs_proj = self.bs_proj or bs
        # (0-d float64 arithmetic on the operands' device; stored as float32, the dtype the three have always had)
        corr = (cross / (sx * sg)).float()
        var_sgd = (sxg * (bs / (bs - 1)) - cross / (bs - 1)).float()
        var_rmm = ((sx * sg - cross) / bs_proj).float()
        if callable(self.callback):
            self.callback(corr, var_sgd, var_rmm, self.step)
        self.step += 1
        self.variance = (corr, var_sgd, var_rmm)


class VarianceEstimator(torch.nn.Module):
    """Wraps a randomized linear layer (anything with ``proj_dim*`` attributes) and evaluates the three quantities
    above on every backward pass; ``callback(corr, var_sgd, var_rmm, step)`` receives them, ``.variance`` keeps the
    last triple.  (The reference stores ``var_sgd`` twice in ``.variance``, fewbit/modules/variance.py:77; here the
    third entry is ``var_rmm``.)

    The copy of a call's input and its row counts travel with that call (``_CatchPair``): a wrapped layer that is called several times
    before one ``backward()`` -- tied weights, a layer applied per segment, a siamese pair -- reports one triple per call, in backward
    order, each of its own (input, gradient) pair; ``state.input`` / ``.grad_output`` / ``.bs`` / ``.bs_proj`` are filled when a pair is
    complete and describe the last backward.  Inside ``torch.utils.checkpoint`` (both modes) a step reports once.  A call that cannot
    reach a backward -- ``no_grad``, ``inference_mode``, nothing requiring grad -- is the wrapped model's call and nothing else: no copy,
    and the state keeps describing the last step that had a gradient."""

    def __init__(self, model: torch.nn.Module, callback: Optional[Callable] = None):
        super().__init__()
        self.model = model
        self.state = _VarianceState(callback)

    @property
    def variance(self):
        return self.state.variance

    def forward(self, input: torch.Tensor, *args, **kwargs):
        # a call that cannot reach a backward (grad mode off, nothing requiring grad) is the model's and nothing else: no copy of the input,
        # and the state keeps describing the last step that had a gradient
        if not (torch.is_grad_enabled() and (input.requires_grad or any(p.requires_grad for p in self.model.parameters()))):
            return self.model(input, *args, **kwargs)
        rows = input.numel() // input.shape[-1]
        bs_proj = projection_dim(rows, getattr(self.model, 'proj_dim_ratio', None), getattr(self.model, 'proj_dim', None),
                                 getattr(self.model, 'proj_dim_max', None), getattr(self.model, 'proj_dim_min', None))
        kept = input.detach().clone()
        output = self.model(input, *args, **kwargs)
        first = output[0] if isinstance(output, tuple) else output
        if not first.requires_grad:
            return output
        # the pair of a call is completed by that call's own node: one module called twice in a step reports two triples, each of its own
        # (input, gradient), in backward order; ``state.input`` / ``.grad_output`` / ``.bs`` / ``.bs_proj`` are those of the last backward
        caught = _CatchPair.apply(first, kept, self.state, rows, bs_proj)
        return (caught, ) + tuple(output[1:]) if isinstance(output, tuple) else caught
