"""A tensor kept in 2, 4 or 8 bits per element for backward: what the quantized nodes (``linear._LinearQuantized``, ``glu._GLUQuantized``,
``glu._GatedMLPQuantized``, the norms of ``norm``) share.  The check of ``bits``; the PyTorch formulation of the packed form of a seed
(``quantize_groups`` / ``decode``: the same groups and the same unbiased rounding as the kernels of fewbit_amd/csrc/fewbit_quant.hip, ``U`` from a
generator, one code per byte; not bit for bit the kernel's); a 2-D tensor kept either way (``keep`` / ``kept_as``); and the products of
gradients with it (``products``), in two terms where the gradient's dtype is too coarse for the decode.  The switch between the kernels and
the PyTorch formulation, and the seeds, are ``linear``'s.
"""
from typing import Optional, Sequence, Tuple

import torch

from . import cabi_x

GROUP = cabi_x.QUANT_GROUP                      # elements (by flat index, or of a row) that share one (lo, step) pair


def check_bits(bits: int) -> None:
    if bits not in cabi_x.QUANT_BITS:
        raise ValueError(f'bits should be 2, 4 or 8, but got {bits}.')


def trains(*tensors: Optional[torch.Tensor]) -> bool:
    """whether a gradient can follow a call: grad mode is on and one of ``tensors`` requires grad (otherwise the call is the plain forward: no seed is
    drawn, nothing is kept, no node is built)"""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def exact_in_eval(module: torch.nn.Module, *tensors: Optional[torch.Tensor]) -> bool:
    """The eval-mode rule of the quantized modules: eval mode is not where activation memory is short, so gradients asked for there are torch's exact
    ones -- nothing is rounded, no seed is drawn"""
    return not module.training and trains(*tensors)


def quantize_groups(flat: torch.Tensor, bits: int, generator: Optional[torch.Generator]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The PyTorch formulation of the packed form: -> (codes, one uint8 per element of the padded groups; lo; step, one per group), in fp32
    (fp64 for a float64 input).  The tail of the last group is filled with the last element, which moves neither its minimum nor its maximum."""
    levels = float(2**bits - 1)
    work = flat.reshape(-1).to(torch.float64 if flat.dtype == torch.float64 else torch.float32)
    pad = -work.numel() % GROUP
    if pad:
        work = torch.cat((work, work[-1:].expand(pad)))
    work = work.view(-1, GROUP)
    lo, hi = work.amin(dim=1, keepdim=True), work.amax(dim=1, keepdim=True)
    span = hi - lo
    poisoned = ~torch.isfinite(span)                                        # (a NaN reaches amin / amax, an infinity makes the span inf or NaN)
    step = span / levels
    inv = torch.where(span > 0, levels / span, torch.zeros_like(span))
    inv = torch.where(torch.isfinite(inv), inv, torch.zeros_like(inv))
    if generator is None:
        u = torch.rand(work.shape, dtype=work.dtype, device=work.device)
    else:
        u = torch.rand(work.shape, dtype=work.dtype, device=generator.device, generator=generator).to(work.device)
    codes = torch.floor((work - lo) * inv + u).clamp_(max=levels)
    codes = torch.where(poisoned, torch.zeros_like(codes), codes).to(torch.uint8)
    nan = torch.full_like(lo, float('nan'))
    return codes.reshape(-1), torch.where(poisoned, nan, lo).reshape(-1), torch.where(poisoned, nan, step).reshape(-1)


def decode(codes: torch.Tensor, lo: torch.Tensor, step: torch.Tensor, rows: int, width: int) -> torch.Tensor:
    """``lo + code * step`` of ``quantize_groups`` as ``rows x width``, each row's padding cut off (a flat tensor: one row); a poisoned group: NaN"""
    values = torch.addcmul(lo[:, None], codes.view(-1, GROUP).to(lo.dtype), step[:, None])
    return values.view(rows, -1)[:, :width]


def keep(flat: torch.Tensor, bits: int, seed, generator: Optional[torch.Generator]) -> tuple:
    """The tensors a node saves to keep the 2-D ``flat`` in ``bits`` bits.  With a ``seed`` (an int, or a device word): ONE uint8 buffer written by the
    kernels (``cabi_x.quant_pack``; a non-contiguous input is packed from a contiguous copy, which lives no longer than this call).  ``seed=None``:
    the codes, lo and step of the PyTorch formulation, drawn from ``generator``."""
    if seed is None:
        return quantize_groups(flat, bits, generator)
    return (cabi_x.quant_pack(flat if flat.is_contiguous() else flat.contiguous(), seed, bits), )


def kept_as(saved: Sequence[torch.Tensor], shape, bits: int, dtype: torch.dtype) -> torch.Tensor:
    """X^ of ``shape`` (2-D) in ``dtype`` from what ``keep`` returned: a transient tensor"""
    count = shape[0] * shape[1]
    if len(saved) == 1:
        return cabi_x.quant_unpack(saved[0], count, bits, dtype).view(shape)
    return decode(*saved, 1, count).view(shape).to(dtype)


def decode_in_two_terms(bits: int, dtype: torch.dtype) -> bool:
    """Whether ``G^T X^`` needs X^ to better than ``dtype``: a bf16 gradient at 8 bits.  There the step, range / 255, is about one bf16 ulp of a
    group's larger elements, and rounding ``lo + code * step`` to bf16 moves an element by up to half an ulp in a direction that does not depend
    on the seed: over many seeds the mean weight gradient then sits several of its standard errors from ``G^T X`` (measured: 8.5, against 3.5
    for the fp32 decode of the same buffers).  At 2 and 4 bits the step is 85 and 17 times larger, and fp16 has eight times bf16's resolution."""
    return bits == 8 and dtype == torch.bfloat16


def two_term_product(g: torch.Tensor, decoded: torch.Tensor) -> torch.Tensor:
    """``g^T decoded`` for a 16-bit ``g`` and an fp32 ``decoded`` on the 16-bit matrix pipe: ``decoded = head + tail`` with ``head`` its rounding to
    the dtype of ``g`` (what ``quant_unpack`` into that dtype gives) and ``tail`` the rounding of the exact remainder.  Both products have to meet
    in fp32 and be rounded once: summed after the first was rounded to 16 bits, that one swallows the second, a fraction of its ulp (measured:
    the deviation stayed).  On the GPU the library GEMM gives fp32 results for 16-bit operands (``out_dtype``): two GEMMs, an fp32 sum, rounded
    by the caller.  Elsewhere ONE GEMM of twice the depth, ``[g; g]^T [head; tail]``.  What is left of the rounding of ``decoded`` is 2^-9 of
    the tail: 2^-18 of an element."""
    return _product_of_two_terms(g, _split_in_two_terms(decoded, g.dtype))


def _split_in_two_terms(decoded: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """``[head; tail]`` of an fp32 ``decoded`` in ``dtype`` (``two_term_product``): split ONCE where several gradients multiply one decode"""
    rows = decoded.shape[0]
    terms = torch.empty((2 * rows, decoded.shape[1]), dtype=dtype, device=decoded.device)
    terms[:rows].copy_(decoded)                                             # head
    torch.sub(decoded, terms[:rows], out=terms[rows:])                      # tail: the difference is exact in fp32, rounded on the store
    return terms


def _product_of_two_terms(g: torch.Tensor, terms: torch.Tensor) -> torch.Tensor:
    rows = terms.shape[0] // 2
    if g.is_cuda:                                                           # two GEMMs with fp32 results: no copy of g, no doubled depth
        with torch.autocast('cuda', enabled=False):
            return torch.mm(g.T, terms[:rows], out_dtype=torch.float32) + torch.mm(g.T, terms[rows:], out_dtype=torch.float32)
    return torch.cat((g, g)).T @ terms


def products(gradients: Sequence[Optional[torch.Tensor]], saved: Sequence[torch.Tensor], shape, bits: int) -> list:
    """``g^T X^`` for every ``g`` of ``gradients`` (2-D, one dtype; None stays None) with the X^ that ``saved`` keeps (``keep``): X^ is decoded ONCE,
    in the gradients' dtype -- under autocast not the input's -- and multiplied in one GEMM each; a bf16 gradient at 8 bits meets an fp32 decode
    split ONCE into two bf16 terms (``decode_in_two_terms``: about twice the time of the other widths).  The caller rounds to the weight's dtype."""
    dtype = next(g.dtype for g in gradients if g is not None)
    if decode_in_two_terms(bits, dtype):
        terms = _split_in_two_terms(kept_as(saved, shape, bits, torch.float32), dtype)
        return [None if g is None else _product_of_two_terms(g, terms) for g in gradients]
    decoded = kept_as(saved, shape, bits, dtype)
    return [None if g is None else g.T @ decoded for g in gradients]
