"""ctypes binding of the companion library ``libfewbit_hipx.so`` (include/fewbit_hipx.h): the entry points added after the C-ABI
of ``libfewbit_hip.so`` was frozen at version 5 (``cabi.SYMBOLS`` stays that list).  Same conventions as ``cabi``: device tensors,
torch's current stream on the tensors' device, no fallback -- a missing library or an unsupported shape raises.  What it binds: the sampled
Fourier transform, the zero-extended and sign-flipped sampled transforms, the column sampling of LinearCRS, the moments of the variance
estimator, the dropout of a seed, the packed form of a seed, the layer norm and the RMS norm that keep the normalized rows of a seed, and the
same two norms with ``residual + dropout(x)`` fused in front, and the product of a gated MLP that keeps the gate and the up of a seed, with the backward that also rebuilds that product from the state, and the cross entropy of a row that keeps the logits as given and one float per row.
"""
import ctypes
import os
from pathlib import Path
from typing import Optional, Tuple

import torch

from .cabi import CONTINUOUS, DTYPES, FewbitHipError, _buffers, _matrix, _on, _planes_dtype, _row_numbers, _same_device, _sampled_call, _seed_arguments, _span, _stream

__all__ = ['LIB_PATH', 'ABI_VERSION', 'REVISION', 'SYMBOLS', 'lib', 'sampled_dft', 'sampled_dft_seeded', 'sampled_dft_workspace_bytes', 'crs_columns',
           'crs_count', 'crs_workspace_bytes', 'crs_gather', 'crs_scatter', 'sampled_rows_ceil', 'sampled_dct_zext', 'sampled_dct_zext_seeded',
           'sampled_dft_zext', 'sampled_dft_zext_seeded', 'sampled_signs', 'sampled_dct_signed', 'sampled_dft_signed', 'moments_workspace_bytes', 'row_moments', 'sum_squares',
           'DROPOUT_SWEEP', 'dropout_threshold', 'dropout_keep', 'dropout_apply', 'QUANT_BITS', 'QUANT_GROUP', 'QUANT_SWEEP', 'quant_bytes', 'quant_pack',
           'quant_unpack', 'quant_pack_host', 'quant_unpack_host', 'NORM_MAX_WIDTH', 'norm_plan', 'norm_state_bytes', 'norm_workspace_bytes', 'norm_state_host',
           'norm_state_unpack_host', 'layer_norm_forward', 'layer_norm_backward', 'rms_norm_forward', 'rms_norm_backward', 'add_layer_norm_forward', 'add_layer_norm_backward',
           'add_rms_norm_forward', 'add_rms_norm_backward', 'GLU_ACTIVATIONS', 'glu_state_bytes', 'glu_state_host', 'glu_forward', 'glu_backward',
           'glu_backward_product', 'CROSS_ENTROPY_MAX_GROUPS', 'cross_entropy_host', 'cross_entropy_forward', 'cross_entropy_backward']

LIB_PATH = Path(os.environ.get('FEWBIT_HIPX_LIB') or Path(__file__).resolve().with_name('libfewbit_hipx.so'))
ABI_VERSION = 1                                # FEWBIT_HIPX_ABI_VERSION this binding was written against
REVISION = 2                                   # FEWBIT_HIPX_REVISION: additions inside ABI version 1 (2: the crs entry points)

_vp, _sz, _i32, _u32, _u64, _dbl, _i64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double, ctypes.c_int64

# every symbol include/fewbit_hipx.h declares: (restype, argtypes).  The ONE list: ``SYMBOLS`` is its keys, ``lib()`` refuses a library that lacks one
# of them and types every one of them from here, so no entry point can be called with ctypes' default conversions.
_SIGNATURES = {
    'fewbit_hipx_abi_version': (_i32, []),
    'fewbit_hipx_last_error': (ctypes.c_char_p, []),
    'fewbit_hipx_sampled_dft_workspace': (_sz, [_i32, _sz, _sz, _sz]),
    'fewbit_hipx_sampled_dft': (_i32, [_i32, _vp, _sz, _sz, _sz, _vp, _sz, _dbl, _i32, _vp, _vp, _sz, _vp]),
    'fewbit_hipx_sampled_dft_seeded': (_i32, [_i32, _vp, _sz, _sz, _sz, _u64, _vp, _sz, _dbl, _i32, _vp, _vp, _sz, _vp]),
    'fewbit_hipx_revision': (_i32, []),
    'fewbit_hipx_crs_columns': (_i32, [_u64, _sz, _sz, _vp, _vp, ctypes.POINTER(_sz)]),
    'fewbit_hipx_crs_workspace': (_sz, [_i32, _sz, _sz, _sz]),
    'fewbit_hipx_crs_gather': (_i32, [_i32, _vp, _sz, _sz, _sz, _u64, _vp, _sz, _sz, _vp, _vp, _sz, _vp]),
    'fewbit_hipx_crs_scatter': (_i32, [_i32, _vp, _sz, _sz, _u64, _vp, _sz, _sz, _vp, _vp, _sz, _vp]),
    # the zero-extended sampled transforms: inside revision 2, recognised by their symbols (checked in lib() with every other name)
    'fewbit_hipx_sampled_rows_ceil': (_sz, [_sz]),
    'fewbit_hipx_sampled_dct_zext': (_i32, [_i32, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _dbl, _vp, _vp, _sz, _vp]),
    'fewbit_hipx_sampled_dct_zext_seeded': (_i32, [_i32, _vp, _sz, _sz, _sz, _sz, _u64, _vp, _sz, _dbl, _vp, _vp, _sz, _vp]),
    'fewbit_hipx_sampled_dft_zext': (_i32, [_i32, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _dbl, _i32, _vp, _vp, _sz, _vp]),
    'fewbit_hipx_sampled_dft_zext_seeded': (_i32, [_i32, _vp, _sz, _sz, _sz, _sz, _u64, _vp, _sz, _dbl, _i32, _vp, _vp, _sz, _vp]),
    # the moments of the variance estimator: inside revision 2 as well, recognised by their symbols
    'fewbit_hipx_moments_workspace': (_sz, [_sz, _sz, _sz]),
    'fewbit_hipx_row_moments': (_i32, [_i32, _vp, _sz, _sz, _i32, _vp, _sz, _sz, _sz, _vp, _vp, _sz, _vp]),
    'fewbit_hipx_sum_squares': (_i32, [_i32, _vp, _sz, _vp, _vp, _sz, _vp]),
    # the dropout of a seed: inside revision 2 as well, recognised by its symbols
    'fewbit_hipx_dropout_threshold': (_i32, [_dbl]),
    'fewbit_hipx_dropout_keep': (_i32, [_u64, _u32, _u64, _sz, _vp]),
    'fewbit_hipx_dropout': (_i32, [_i32, _vp, _vp, _vp, _sz, _u64, _u64, _vp, _u32, _vp]),
    # the sampled transforms with the signs of a seed: inside revision 2 as well, recognised by their symbols
    'fewbit_hipx_sampled_signs': (_i32, [_u64, _u64, _sz, _vp]),
    'fewbit_hipx_sampled_dct_signed': (_i32, [_i32, _vp, _sz, _sz, _sz, _sz, _u64, _vp, _sz, _dbl, _vp, _vp, _sz, _vp]),
    'fewbit_hipx_sampled_dft_signed': (_i32, [_i32, _vp, _sz, _sz, _sz, _sz, _u64, _vp, _sz, _dbl, _i32, _vp, _vp, _sz, _vp]),
    # the packed form of a seed: inside revision 2 as well, recognised by its symbols
    'fewbit_hipx_quant_bytes': (_sz, [_sz, _i32]),
    'fewbit_hipx_quant_pack_host': (_i32, [_vp, _sz, _i32, _u64, _vp]),
    'fewbit_hipx_quant_unpack_host': (_i32, [_vp, _sz, _i32, _vp]),
    'fewbit_hipx_quant_pack': (_i32, [_i32, _vp, _sz, _i32, _u64, _vp, _vp, _sz, _vp]),
    'fewbit_hipx_quant_unpack': (_i32, [_vp, _sz, _i32, _i32, _vp, _vp]),
    # the normalized rows of a seed (the layer norm): inside revision 2 as well, recognised by its symbols
    'fewbit_hipx_norm_state_bytes': (_sz, [_sz, _sz, _i32]),
    'fewbit_hipx_norm_workspace': (_sz, [_sz, _sz]),
    'fewbit_hipx_norm_state_host': (_i32, [_vp, _sz, _sz, _i32, _u64, _vp]),
    'fewbit_hipx_norm_state_unpack_host': (_i32, [_vp, _sz, _sz, _i32, _vp]),
    'fewbit_hipx_layer_norm_forward': (_i32, [_i32, _vp, _sz, _sz, _vp, _vp, _dbl, _i32, _u64, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    'fewbit_hipx_layer_norm_backward': (_i32, [_i32, _vp, _vp, _vp, _vp, _sz, _sz, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    # the un-centred rows (the RMS norm): inside revision 2 as well, recognised by its symbols
    'fewbit_hipx_rms_norm_forward': (_i32, [_i32, _vp, _sz, _sz, _vp, _dbl, _i32, _u64, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    'fewbit_hipx_rms_norm_backward': (_i32, [_i32, _vp, _vp, _vp, _vp, _sz, _sz, _i32, _vp, _vp, _vp, _sz, _vp]),
    # the sum of a seed in front of the norm (residual + dropout(x), then either norm): inside revision 2 as well, recognised by its symbols
    'fewbit_hipx_add_layer_norm_forward': (_i32, [_i32, _vp, _vp, _sz, _sz, _vp, _vp, _dbl, _i32, _u64, _vp, _u32, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    'fewbit_hipx_add_layer_norm_backward': (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _i32, _u64, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'fewbit_hipx_add_rms_norm_forward': (_i32, [_i32, _vp, _vp, _sz, _sz, _vp, _dbl, _i32, _u64, _vp, _u32, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    'fewbit_hipx_add_rms_norm_backward': (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _i32, _u64, _vp, _u32, _vp, _vp, _vp, _vp, _sz, _vp]),
    # the gate and the up of a seed (the product of a gated MLP): inside revision 2 as well, recognised by its symbols
    'fewbit_hipx_glu_state_bytes': (_sz, [_sz, _i32]),
    'fewbit_hipx_glu_state_host': (_i32, [_vp, _vp, _sz, _i32, _u64, _vp]),
    'fewbit_hipx_glu_forward': (_i32, [_i32, _i32, _vp, _sz, _vp, _sz, _sz, _sz, _i32, _u64, _vp, _vp, _vp, _sz, _vp]),
    'fewbit_hipx_glu_backward': (_i32, [_i32, _i32, _vp, _vp, _sz, _sz, _i32, _vp, _sz, _vp, _sz, _vp]),
    # the same backward that also rebuilds the product from the decodes (the gated MLP as one node): inside revision 2 as well, recognised by its symbol
    'fewbit_hipx_glu_backward_product': (_i32, [_i32, _i32, _vp, _vp, _sz, _sz, _i32, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    # the loss of a row (the cross entropy that keeps the logits as given and one float per row): inside revision 2 as well, recognised by its symbols
    'fewbit_hipx_cross_entropy_host': (_i32, [_vp, _vp, _sz, _sz, _i64, _vp, _vp, _vp, _vp]),
    'fewbit_hipx_cross_entropy_forward': (_i32, [_i32, _vp, _sz, _sz, _sz, _vp, _i64, _vp, _vp, _vp]),
    'fewbit_hipx_cross_entropy_backward': (_i32, [_i32, _vp, _sz, _sz, _sz, _vp, _i64, _vp, _vp, _sz, _vp, _sz, _vp]),
}
SYMBOLS = tuple(_SIGNATURES)

_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise FewbitHipError(f'{LIB_PATH} is missing: build it with `make -C fewbit_amd/csrc` '
                                 '(or `python -c "import __graft_entry__ as g; g.build()"`)')
        L = ctypes.CDLL(str(LIB_PATH))
        missing = [name for name in SYMBOLS if not hasattr(L, name)]
        if missing:
            raise FewbitHipError(f'{LIB_PATH} lacks {", ".join(missing)} (an older revision of the library): rebuild it (make -C fewbit_amd/csrc)')
        have = L.fewbit_hipx_abi_version()                    # (`int f(void)`, as is the revision: what ctypes assumes of an untyped symbol)
        if have < ABI_VERSION:
            raise FewbitHipError(f'{LIB_PATH} has ABI version {have}, this binding needs {ABI_VERSION}: rebuild it (make -C fewbit_amd/csrc)')
        if L.fewbit_hipx_revision() < REVISION:
            raise FewbitHipError(f'{LIB_PATH} has revision {L.fewbit_hipx_revision()}, this binding needs {REVISION}: rebuild it (make -C fewbit_amd/csrc)')
        for name, (restype, argtypes) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def _check(rc: int):
    if rc != 0:
        raise FewbitHipError(f'fewbit_hipx error {rc}: {lib().fewbit_hipx_last_error().decode()}')


# ---- sampled Fourier transform (fewbit_amd/csrc/fewbit_dft.hip): out = scale * fft(m, dim=0, norm='ortho')[idx] as two planes -----
def sampled_dft_workspace_bytes(rows: int, features: int, proj: int, dtype: torch.dtype = torch.bfloat16) -> int:
    """bytes of scratch a ``sampled_dft`` call needs (the formula of ``cabi.sampled_dct_workspace_bytes``); 0 = this shape has no kernel
    (rows not of ``cabi.SAMPLED_ROWS``, or a dtype other than fp32 / fp16 / bf16)"""
    if dtype not in DTYPES:
        return 0
    return lib().fewbit_hipx_sampled_dft_workspace(DTYPES[dtype], rows, features, proj)


_DFT = ('sampled_dft', sampled_dft_workspace_bytes, _check, (2, ), '2 x proj x features tensor of out_dtype')


def sampled_dft(m: torch.Tensor, idx: torch.Tensor, scale: float = 1.0, out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    """``scale * torch.fft.fft(m, dim=0, norm='ortho')[idx]`` for a 2-D ``m`` (rows x features, unit stride along the features) whose row
    count is one of ``cabi.SAMPLED_ROWS``; ``idx``: int64 row numbers on the device of ``m``.
    fp32 arithmetic.  Returns a ``(2, proj, features)`` tensor of ``out_dtype`` (torch.float32 or the dtype of ``m``, the default):
    ``[0]`` the real part, ``[1]`` the imaginary part.

    Features ``(2c, 2c + 1)`` are transformed as one complex column: the rounding error of column ``c`` scales with the RMS of the pair
    ``(c, c ^ 1)``, and a NaN or Inf in one column makes its partner non-finite too (other columns stay bit for bit as they are).
    torch.fft keeps every column apart."""
    proj, odt = _row_numbers(idx, m), _planes_dtype(m, out_dtype)
    return _sampled_call(_DFT, m, proj, odt, out, workspace, (idx, ), stream,
                         lambda head, tail: lib().fewbit_hipx_sampled_dft(*head, idx.data_ptr(), proj, scale, DTYPES[odt], *tail))


def sampled_dft_seeded(m: torch.Tensor, proj: int, seed, scale: float = 1.0, out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None,
                       workspace: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    """``sampled_dft(m, cabi.sampled_rows(seed, rows, proj))`` without the array of row numbers: the rows are a function of ``seed`` that the
    kernel evaluates itself (the rows ``cabi.sampled_dct_seeded`` samples).  ``seed``: an int, or a one-element int64 tensor on the device of
    ``m`` whose value is read when the kernel runs (``cabi.next_sketch_seed``: a launch recorded into a hipGraph then samples fresh rows on
    every replay).  The pair contract of ``sampled_dft`` holds: column ``c``'s error scales with the RMS of the pair ``(c, c ^ 1)``, a
    non-finite value reaches the partner."""
    (value, word, others), odt = _seed_arguments(seed), _planes_dtype(m, out_dtype)
    return _sampled_call(_DFT, m, proj, odt, out, workspace, others, stream,
                         lambda head, tail: lib().fewbit_hipx_sampled_dft_seeded(*head, value, word, proj, scale, DTYPES[odt], *tail))


# ---- the sampled transforms at any row count: x is transformed as if zero rows followed it, up to a supported row count -------------------
def sampled_rows_ceil(rows: int) -> int:
    """The smallest row count of ``cabi.SAMPLED_ROWS`` that is ``>= rows`` (256 for 1 .. 256); 0 for ``rows = 0`` and beyond 262144.
    Evaluated on the host from the table the kernels are dispatched by; no GPU needed."""
    if rows < 0:
        raise FewbitHipError(f'rows must not be negative (got {rows})')
    return lib().fewbit_hipx_sampled_rows_ceil(rows)


# (the workspace of a zero-extended call is the plain formula at ``rows``; the DCT's is asked of this library too, which owns its kernels)
_DCT_ZEXT = ('sampled_dct_zext', sampled_dft_workspace_bytes, _check, (), 'proj x features tensor of the dtype of x')
_DFT_ZEXT = ('sampled_dft_zext', sampled_dft_workspace_bytes, _check, (2, ), '2 x proj x features tensor of out_dtype')


def sampled_dct_zext(x: torch.Tensor, rows: int, idx: torch.Tensor, scale: float = 1.0, out: Optional[torch.Tensor] = None,
                     workspace: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    """``scale * dct(cat(x, zeros), dim=0, norm='ortho')[idx]`` at length ``rows`` (a row count of ``cabi.SAMPLED_ROWS``, e.g.
    ``sampled_rows_ceil(x.shape[0])``) for a 2-D ``x`` of 1 .. ``rows`` rows, without the padded copy: the missing rows are zeros the kernel
    never loads, and nothing behind the last row of ``x`` is read.  ``idx``: int64 row numbers in ``[0, rows)`` on the device of ``x``.  Bit
    for bit ``cabi.sampled_dct`` of the zero-filled copy; the pair contract of ``cabi.sampled_dct`` holds.

    With rows drawn uniformly from ``[0, rows)`` and ``scale = sqrt(rows / p)`` this is a sketch ``S x`` with ``E[S^T S] = I`` over the rows of
    ``x`` (include/fewbit_hipx.h) -- unbiased like the layer's own, but not the reference's ``dct(x)[idx]`` at length ``x.shape[0]``."""
    proj = _row_numbers(idx, x, 'x')
    return _sampled_call(_DCT_ZEXT, x, proj, x.dtype, out, workspace, (idx, ), stream,
                         lambda head, tail: lib().fewbit_hipx_sampled_dct_zext(*head, idx.data_ptr(), proj, scale, *tail), rows)


def sampled_dct_zext_seeded(x: torch.Tensor, rows: int, p: int, seed, scale: float = 1.0, out: Optional[torch.Tensor] = None,
                            workspace: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    """``sampled_dct_zext(x, rows, cabi.sampled_rows(seed, rows, p))`` without the array of row numbers (``seed``: an int, or a one-element
    int64 tensor on the device of ``x`` that is read when the kernel runs, as in ``cabi.sampled_dct_seeded``)"""
    value, word, others = _seed_arguments(seed)
    return _sampled_call(_DCT_ZEXT, x, p, x.dtype, out, workspace, others, stream,
                         lambda head, tail: lib().fewbit_hipx_sampled_dct_zext_seeded(*head, value, word, p, scale, *tail), rows)


def sampled_dft_zext(x: torch.Tensor, rows: int, idx: torch.Tensor, scale: float = 1.0, out_dtype: Optional[torch.dtype] = None,
                     out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    """``scale * torch.fft.fft(cat(x, zeros), dim=0, norm='ortho')[idx]`` at length ``rows`` as a ``(2, proj, features)`` tensor (real plane,
    imaginary plane) of ``out_dtype``: ``sampled_dft`` of the zero-filled copy, bit for bit, without the copy (see ``sampled_dct_zext``)"""
    proj, odt = _row_numbers(idx, x, 'x'), _planes_dtype(x, out_dtype, 'x')
    return _sampled_call(_DFT_ZEXT, x, proj, odt, out, workspace, (idx, ), stream,
                         lambda head, tail: lib().fewbit_hipx_sampled_dft_zext(*head, idx.data_ptr(), proj, scale, DTYPES[odt], *tail), rows)


def sampled_dft_zext_seeded(x: torch.Tensor, rows: int, p: int, seed, scale: float = 1.0, out_dtype: Optional[torch.dtype] = None,
                            out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    """``sampled_dft_zext(x, rows, cabi.sampled_rows(seed, rows, p))`` without the array of row numbers (``seed`` as in ``sampled_dft_seeded``)"""
    (value, word, others), odt = _seed_arguments(seed), _planes_dtype(x, out_dtype, 'x')
    return _sampled_call(_DFT_ZEXT, x, p, odt, out, workspace, others, stream,
                         lambda head, tail: lib().fewbit_hipx_sampled_dft_zext_seeded(*head, value, word, p, scale, DTYPES[odt], *tail), rows)


# ---- the sampled transforms behind a random sign per row (fewbit_amd/csrc/fewbit_signed.hip): scale * T(D x)[rows of the seed] -----------------
_DCT_SIGNED = ('sampled_dct_signed', sampled_dft_workspace_bytes, _check, (), 'proj x features tensor of the dtype of x')
_DFT_SIGNED = ('sampled_dft_signed', sampled_dft_workspace_bytes, _check, (2, ), '2 x proj x features tensor of out_dtype')


def sampled_signs(seed: int, rows: int, first: int = 0) -> torch.Tensor:
    """The signs ``sampled_dct_signed`` / ``sampled_dft_signed`` give the rows ``first .. first + rows`` of their input for ``seed``: a host
    bool tensor, True where the row is negated.  The definition is include/fewbit_hipx.h's ("the signs of a seed"); evaluated on the host,
    no GPU needed; ``first`` may be any row number below 2^64."""
    if rows < 0 or first < 0:
        raise FewbitHipError(f'rows and first must not be negative (got {rows}, {first})')
    flip = torch.empty(rows, dtype=torch.uint8)
    _check(lib().fewbit_hipx_sampled_signs(seed & 0xffffffffffffffff, first & 0xffffffffffffffff, rows, flip.data_ptr()))
    return flip.bool()


def sampled_dct_signed(x: torch.Tensor, rows: int, p: int, seed, scale: float = 1.0, out: Optional[torch.Tensor] = None,
                       workspace: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    """``sampled_dct_zext_seeded`` of ``x`` with the rows of ``sampled_signs(seed, x.shape[0])`` negated, bit for bit, without the negated
    copy: the kernel evaluates the signs itself and flips the sign bits of the rows it has just loaded.  ``rows``: the length of the
    transform, a row count of ``cabi.SAMPLED_ROWS`` (``x.shape[0]`` itself where it is one).  ``seed``: an int, or a one-element int64 tensor
    on the device of ``x`` that is read when the kernel runs -- for the sampled rows and the signs alike, so a launch recorded into a hipGraph
    draws both afresh on every replay."""
    value, word, others = _seed_arguments(seed)
    return _sampled_call(_DCT_SIGNED, x, p, x.dtype, out, workspace, others, stream,
                         lambda head, tail: lib().fewbit_hipx_sampled_dct_signed(*head, value, word, p, scale, *tail), rows)


def sampled_dft_signed(x: torch.Tensor, rows: int, p: int, seed, scale: float = 1.0, out_dtype: Optional[torch.dtype] = None,
                       out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    """``sampled_dft_zext_seeded`` of ``x`` with the rows of ``sampled_signs(seed, x.shape[0])`` negated, bit for bit (see
    ``sampled_dct_signed``); a ``(2, p, features)`` tensor of ``out_dtype``"""
    (value, word, others), odt = _seed_arguments(seed), _planes_dtype(x, out_dtype, 'x')
    return _sampled_call(_DFT_SIGNED, x, p, odt, out, workspace, others, stream,
                         lambda head, tail: lib().fewbit_hipx_sampled_dft_signed(*head, value, word, p, scale, DTYPES[odt], *tail), rows)


# ---- column sampling of LinearCRS (fewbit_amd/csrc/fewbit_crs.hip): the columns of a seed, the gather of forward, the scatter of backward ----
def crs_count(seed: int, in_features: int, nopairs: int) -> int:
    """``m``, the number of distinct columns among the ``nopairs`` draws of ``seed`` (evaluated on the host; no GPU needed)"""
    m = ctypes.c_size_t(0)
    _check(lib().fewbit_hipx_crs_columns(seed & 0xffffffffffffffff, in_features, nopairs, None, None, ctypes.byref(m)))
    return m.value


def crs_columns(seed: int, in_features: int, nopairs: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The columns ``crs_gather`` keeps for ``seed``: (``cols``, ascending distinct column numbers as a host int64 tensor; ``count``, how often
    each was drawn, int32; ``count.sum() == nopairs``).  The definition is include/fewbit_hipx.h's; evaluated on the host, no GPU needed."""
    room = min(nopairs, in_features)
    cols, count, m = torch.empty(room, dtype=torch.int64), torch.empty(room, dtype=torch.int32), ctypes.c_size_t(0)
    _check(lib().fewbit_hipx_crs_columns(seed & 0xffffffffffffffff, in_features, nopairs, cols.data_ptr(), count.data_ptr(), ctypes.byref(m)))
    return cols[:m.value], count[:m.value]


def crs_workspace_bytes(rows: int, in_features: int, nopairs: int, dtype: torch.dtype = torch.bfloat16) -> int:
    """bytes of scratch a ``crs_gather`` / ``crs_scatter`` call needs; 0 = no kernel (a dtype other than fp32 / fp16 / bf16, no rows, or
    ``in_features`` / ``nopairs`` outside the range include/fewbit_hipx.h states)"""
    if dtype not in DTYPES:
        return 0
    return lib().fewbit_hipx_crs_workspace(DTYPES[dtype], rows, in_features, nopairs)


def _crs_call(name: str, src: torch.Tensor, seed, in_features: int, nopairs: int, shape, out: Optional[torch.Tensor], workspace: Optional[torch.Tensor],
              launch) -> torch.Tensor:
    rows = src.shape[0]
    need = crs_workspace_bytes(rows, in_features, nopairs, src.dtype)
    if need == 0:
        raise FewbitHipError(f'{name}: no kernel for {rows} rows, in_features = {in_features}, nopairs = {nopairs} of {src.dtype}')
    value, word, others = _seed_arguments(seed)
    with _on(src.device):
        out, workspace = _buffers(src, others, out, shape, src.dtype, f'{" x ".join(map(str, shape))} tensor of the dtype of the input', workspace, need)
        _check(launch(DTYPES[src.dtype], src.data_ptr(), value, word, out.data_ptr(), *_span(workspace), _stream(None, src.device)))
    return out


def crs_gather(x: torch.Tensor, seed, nopairs: int, cap: Optional[int] = None, out: Optional[torch.Tensor] = None,
               workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``(x.float()[:, cols] * scale).to(x.dtype)`` padded with zero columns to ``cap`` columns, for the columns of ``seed`` (``crs_columns``;
    ``scale = count * in_features / nopairs``) and a 2-D ``x`` (rows x in_features, unit stride along the features).  ``seed``: an int -- then
    ``cap`` defaults to ``m``, the number of distinct columns, evaluated on the host -- or a one-element int64 tensor on the device of ``x``
    that is read when the kernel runs (``cabi.next_sketch_seed``; a launch recorded into a hipGraph draws fresh columns on every replay) --
    then ``cap`` defaults to ``min(nopairs, in_features)``, which no draw exceeds.  Nothing is read back from the device."""
    rows, in_features, ld = _matrix(x)
    if cap is None:
        cap = min(nopairs, in_features) if isinstance(seed, torch.Tensor) else crs_count(seed, in_features, nopairs)
    return _crs_call('crs_gather', x, seed, in_features, nopairs, (rows, cap), out, workspace, lambda dt, xp, value, word, op, wp, wb, st: lib().fewbit_hipx_crs_gather(
        dt, xp, rows, in_features, ld, value, word, nopairs, cap, op, wp, wb, st))


def crs_scatter(t: torch.Tensor, seed, in_features: int, nopairs: int, out: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The ``out_features x in_features`` weight gradient of the columns of ``seed`` from ``t`` (``out_features x cap``, contiguous; the product
    ``G^T kept`` of a ``crs_gather`` result of the same ``seed`` and ``nopairs``): column ``cols[j]`` is ``t[:, j]``, every other entry is +0.
    All of the result is written in one pass."""
    if t.dim() != 2 or not t.is_contiguous():
        raise FewbitHipError('t must be a contiguous 2-D tensor')
    _matrix(t)
    out_features, cap = t.shape
    return _crs_call('crs_scatter', t, seed, in_features, nopairs, (out_features, in_features), out, workspace,
                     lambda dt, tp, value, word, op, wp, wb, st: lib().fewbit_hipx_crs_scatter(dt, tp, out_features, cap, value, word, in_features, nopairs, op, wp, wb, st))


# ---- the moments of the variance estimator (fewbit_amd/csrc/fewbit_moments.hip): sums of squares in fp64, one read of every element ----------
def moments_workspace_bytes(rows: int, n: int = 1, m: int = 1) -> int:
    """bytes of scratch a ``row_moments`` call on ``rows`` rows of ``n`` and ``m`` columns needs -- and a ``sum_squares`` call on ``rows``
    elements, with ``n = m = 1``; 0 = no kernel (an extent of 0 or beyond the caps include/fewbit_hipx.h states)"""
    if min(rows, n, m) < 0:
        return 0
    return lib().fewbit_hipx_moments_workspace(rows, n, m)


def _rows_of(t: torch.Tensor, what: str) -> torch.Tensor:
    """``t`` as the kernels take it: unit stride along the columns and a row stride that skips no row backwards; anything else as a copy"""
    if t.dim() != 2:
        raise FewbitHipError(f'{what} must be 2-D (got {t.dim()} dimensions)')
    ok = (t.shape[1] <= 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1])
    return t if ok else t.contiguous()


def _moments_call(first: torch.Tensor, others, count: int, out: Optional[torch.Tensor], workspace: Optional[torch.Tensor], rows: int, n: int,
                  m: int, launch) -> torch.Tensor:
    need = moments_workspace_bytes(rows, n, m)
    with _on(first.device):
        out, workspace = _buffers(first, others, out, (count, ), torch.float64, f'float64 tensor of {count} element{"s" if count > 1 else ""}', workspace, need)
        if workspace is None:                                   # (need == 0: the library names the offending extent)
            workspace = torch.empty(0, dtype=torch.uint8, device=first.device)
        _check(launch(out.data_ptr(), *_span(workspace), _stream(None, first.device)))
    return out


def row_moments(x: torch.Tensor, g: torch.Tensor, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``(sx, sg, sxg) = (sum_b |x_b|^2, sum_b |g_b|^2, sum_b |x_b|^2 |g_b|^2)`` of the rows of ``x`` (B x n) and ``g`` (B x m) as a float64
    tensor of 3 elements on their device.  The dtypes (fp32 / fp16 / bf16) are independent.  Every element is read once and squared exactly,
    every sum is fp64 in a fixed order: the same arguments give the same bits, each result is within ``B * max(n, m) * 2^-53`` relative
    of the exact value.  Rows may be strided (``stride(1) == 1``, ``stride(0) >= columns``: no padding element is read); any other layout is
    made contiguous first.  Enqueued on torch's current stream of that device; nothing is read back."""
    x, g = _rows_of(x, 'x'), _rows_of(g, 'g')
    (rows, n, ldx), (rows_g, m, ldg) = _matrix(x), _matrix(g)
    if rows_g != rows:
        raise FewbitHipError(f'x and g must have the same number of rows (got {rows} and {rows_g})')
    return _moments_call(x, (g, ), 3, out, workspace, rows, n, m, lambda op, wp, wb, st: lib().fewbit_hipx_row_moments(
        DTYPES[x.dtype], x.data_ptr(), n, ldx, DTYPES[g.dtype], g.data_ptr(), m, ldg, rows, op, wp, wb, st))


def sum_squares(t: torch.Tensor, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``sum(t^2)`` over all elements of ``t`` (fp32 / fp16 / bf16, any shape; made contiguous if it is not) as a float64 tensor of 1 element
    on its device: the arithmetic, the fixed order and the workspace of ``row_moments`` (within ``t.numel() * 2^-53`` relative)."""
    if t.device.type != 'cuda':
        raise FewbitHipError(f't must live on the GPU (got {t.device})')
    if t.dtype not in DTYPES:
        raise FewbitHipError(f'unsupported dtype {t.dtype}')
    t = t if t.is_contiguous() else t.contiguous()
    count = t.numel()
    return _moments_call(t, (), 1, out, workspace, count, 1, 1,
                         lambda op, wp, wb, st: lib().fewbit_hipx_sum_squares(DTYPES[t.dtype], t.data_ptr(), count, op, wp, wb, st))


# ---- dropout whose mask is a function of a seed (fewbit_amd/csrc/fewbit_dropout.hip): nothing is kept for backward but the seed -------------
DROPOUT_SWEEP = 1 << 22                         # elements one sweep of the launch plan covers (2048 workgroups x 256 lanes x 8); beyond it lanes loop


def dropout_threshold(p: float) -> int:
    """``T``, the threshold of drop probability ``p``: the nearest integer to ``p * 65536`` (ties to even).  An element is dropped with
    probability ``T / 65536`` exactly.  ``p`` outside [0, 1] (NaN included) is refused.  Evaluated on the host; no GPU needed."""
    t = lib().fewbit_hipx_dropout_threshold(float(p))
    if t < 0:
        raise FewbitHipError(f'dropout probability has to be between 0 and 1, but got {p}')
    return t


def dropout_keep(seed: int, n: int, p: float, first: int = 0) -> torch.Tensor:
    """The mask ``dropout_apply`` uses for ``seed``: ``keep(first + j)`` for ``j < n`` as a host bool tensor (True: the element is kept).  The
    definition is include/fewbit_hipx.h's ("the mask of a seed"); evaluated on the host, no GPU needed; ``first`` may be any index."""
    keep = torch.empty(n, dtype=torch.uint8)
    _check(lib().fewbit_hipx_dropout_keep(seed & 0xffffffffffffffff, dropout_threshold(p), first, n, keep.data_ptr()))
    return keep.bool()


def dropout_apply(src: torch.Tensor, seed, p: float, addend: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, first: int = 0,
                  stream: Optional[int] = None) -> torch.Tensor:
    """``where(keep, (src.float() * scale [+ addend.float()]).to(dtype), addend or 0)`` for the mask of ``seed`` (``dropout_keep``) in ONE
    launch: ``scale = float32(65536 / (65536 - T))`` with ``T = dropout_threshold(p)``.  Forward (``src = x``) and backward (``src = gy``, no
    addend) of a dropout that keeps only its seed.  ``src``, ``addend`` and ``out``: contiguous fp32 / fp16 / bf16 GPU tensors of one shape and
    dtype; ``out`` may BE ``src`` or ``addend`` (the same memory exactly).  ``seed``: an int, or a one-element int64 tensor on the device of
    ``src`` that is read when the kernel runs (``cabi.next_sketch_seed``: a launch recorded into a hipGraph draws a fresh mask on every
    replay).  ``first``: the flat index of ``src``'s first element in the logical tensor whose mask is drawn, a multiple of 8 (a shard of a
    tensor passes its offset).  A dropped element is +0 (the addend's bits with an addend) even where ``src`` holds inf or NaN."""
    if src.device.type != 'cuda':
        raise FewbitHipError(f'src must live on the GPU (got {src.device})')
    if src.dtype not in DTYPES:
        raise FewbitHipError(f'unsupported dtype {src.dtype}')
    if not src.is_contiguous():
        raise FewbitHipError('src must be contiguous')
    if addend is not None and (addend.shape != src.shape or addend.dtype != src.dtype or not addend.is_contiguous()):
        raise FewbitHipError('addend must be a contiguous tensor of the shape and dtype of src')
    threshold = dropout_threshold(p)
    value, word, others = _seed_arguments(seed)
    with _on(src.device):
        out, _ = _buffers(src, others + (() if addend is None else (addend, )), out, src.shape, src.dtype, 'tensor of the shape and dtype of src', None, 0)
        _check(lib().fewbit_hipx_dropout(DTYPES[src.dtype], src.data_ptr(), None if addend is None else addend.data_ptr(), out.data_ptr(), src.numel(), first,
                                         value, word, threshold, _stream(stream, src.device)))
    return out


# ---- a tensor kept in 2, 4 or 8 bits per element (fewbit_amd/csrc/fewbit_quant.hip): the packed form of a seed, what QuantizedLinear keeps ------
QUANT_BITS = (2, 4, 8)
QUANT_GROUP = 64                                # elements that share one (lo, step) pair
QUANT_SWEEP = 1 << 22                           # elements one sweep of the launch plan covers (2048 workgroups x 256 lanes x 8); beyond it lanes loop


def quant_bytes(n: int, bits: int) -> int:
    """Bytes of the packed form of ``n`` elements at ``bits`` bits: ``8 * ceil(n / 64) + bits * ceil(n / 8)``; 0 for ``bits`` other than 2, 4, 8
    and for ``n`` outside 1 .. 2^36.  Evaluated on the host; no GPU needed."""
    if n < 0:
        return 0
    return lib().fewbit_hipx_quant_bytes(n, bits)


_QUANT = (quant_bytes, 'no packed form for {} elements (1 .. 2^36 are supported)')


def _size(family, name: str, bits: int, *extents: int) -> int:
    """Bytes of what ``name`` keeps at ``extents``: ``family`` is (the library's size query, the refusal of a size of zero in the family's own words)"""
    query, refusal = family
    if bits not in QUANT_BITS:
        raise FewbitHipError(f'{name}: bits must be 2, 4 or 8 (got {bits})')
    need = query(*extents, bits)
    if extents[0] != 0 and need == 0:
        raise FewbitHipError(f'{name}: {refusal.format(*extents)}')
    return need


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _state_to_write(state: Optional[torch.Tensor], keep: bool, need: int, device, what: str = 'state') -> Optional[torch.Tensor]:
    """the state buffer of a forward: a new one of ``need`` bytes, or the given one checked (the library checks its size), or None with ``keep=False``"""
    if not keep:
        return None
    if state is None:
        return torch.empty(need, dtype=torch.uint8, device=device)
    if state.dtype != torch.uint8 or state.dim() != 1 or not state.is_contiguous():
        raise FewbitHipError(f'{what} must be a contiguous 1-D uint8 tensor')
    return state


def _state_to_read(state: torch.Tensor, need: int, what: str = 'state', host: bool = False) -> None:
    """the state given to a backward or, with ``host``, to a host decode"""
    if (host and state.device.type != 'cpu') or state.dtype != torch.uint8 or not state.is_contiguous() or state.numel() < need:
        raise FewbitHipError(f'{what} must be a contiguous {"host " if host else ""}uint8 tensor of at least {need} bytes')


def quant_pack_host(values: torch.Tensor, seed: int, bits: int) -> torch.Tensor:
    """The buffer ``quant_pack`` writes for ``seed``, evaluated on the host: ``values`` (any shape; taken as contiguous fp32, so pass the
    values of a 16-bit tensor as ``.float()``) -> a host uint8 tensor of ``quant_bytes(values.numel(), bits)`` bytes.  The definition is
    include/fewbit_hipx.h's ("the packed form of a seed"); no GPU needed."""
    x = values.detach().to(device='cpu', dtype=torch.float32).contiguous()
    out = torch.empty(_size(_QUANT, 'quant_pack_host', bits, x.numel()), dtype=torch.uint8)
    _check(lib().fewbit_hipx_quant_pack_host(x.data_ptr(), x.numel(), bits, seed & 0xffffffffffffffff, out.data_ptr()))
    return out


def quant_unpack_host(packed: torch.Tensor, n: int, bits: int) -> torch.Tensor:
    """The fp32 decode of a packed buffer on the host: a float32 tensor of ``n`` elements (``fma(code, step, lo)``; a poisoned group: NaN)"""
    _state_to_read(packed, _size(_QUANT, 'quant_unpack_host', bits, n), 'packed', host=True)
    out = torch.empty(n, dtype=torch.float32)
    _check(lib().fewbit_hipx_quant_unpack_host(packed.data_ptr(), n, bits, out.data_ptr()))
    return out


def quant_pack(x: torch.Tensor, seed, bits: int, out: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    """``x`` (a contiguous fp32 / fp16 / bf16 GPU tensor of any shape, taken by flat index) in ``bits`` bits per element with unbiased
    stochastic rounding, in ONE launch: a uint8 tensor of ``quant_bytes(x.numel(), bits)`` bytes -- per group of 64 elements ``lo`` and
    ``step = (hi - lo) / (2^bits - 1)`` as fp32, then the codes ``min(L, floor((x - lo) / step + U))``, ``U`` drawn from ``seed``.
    ``seed``: an int, or a one-element int64 tensor on the device of ``x`` that is read when the kernel runs (``cabi.next_sketch_seed``: a
    launch recorded into a hipGraph rounds afresh on every replay).  ``quant_pack_host`` gives the same bytes for the same seed.  ``out``: a
    contiguous uint8 tensor of at least that many bytes (8-byte aligned); only the first ``quant_bytes`` bytes are written."""
    if x.device.type != 'cuda':
        raise FewbitHipError(f'x must live on the GPU (got {x.device})')
    if x.dtype not in DTYPES:
        raise FewbitHipError(f'unsupported dtype {x.dtype}')
    if not x.is_contiguous():
        raise FewbitHipError('x must be contiguous')
    need = _size(_QUANT, 'quant_pack', bits, x.numel())
    value, word, others = _seed_arguments(seed)
    with _on(x.device):
        out = _state_to_write(out, True, need, x.device, 'out')
        _same_device(x, out, *others)
        _check(lib().fewbit_hipx_quant_pack(DTYPES[x.dtype], x.data_ptr(), x.numel(), bits, value, word, out.data_ptr(), out.numel(),
                                            _stream(stream, x.device)))
    return out


def quant_unpack(packed: torch.Tensor, n: int, bits: int, dtype: torch.dtype, out: Optional[torch.Tensor] = None,
                 stream: Optional[int] = None) -> torch.Tensor:
    """The decode of a ``quant_pack`` buffer in ONE launch: ``n`` elements of ``dtype`` (fp32 / fp16 / bf16, independent of the dtype that was
    packed), each ``fma(code, step, lo)`` in fp32 rounded once to ``dtype``; a poisoned group decodes to NaN.  ``out``: a contiguous tensor of
    ``n`` elements of ``dtype`` (any shape)."""
    if packed.device.type != 'cuda':
        raise FewbitHipError(f'packed must live on the GPU (got {packed.device})')
    if dtype not in DTYPES:
        raise FewbitHipError(f'unsupported dtype {dtype}')
    _state_to_read(packed, _size(_QUANT, 'quant_unpack', bits, n), 'packed')
    with _on(packed.device):
        if out is None:
            out = torch.empty(n, dtype=dtype, device=packed.device)
        elif out.numel() != n or out.dtype != dtype or not out.is_contiguous():
            raise FewbitHipError(f'out must be a contiguous tensor of {n} elements of {dtype}')
        _same_device(packed, out)
        _check(lib().fewbit_hipx_quant_unpack(packed.data_ptr(), n, bits, DTYPES[dtype], out.data_ptr(), _stream(stream, packed.device)))
    return out


# ---- the layer norm and the RMS norm that keep their normalized rows in 2, 4 or 8 bits (fewbit_amd/csrc/fewbit_norm.hip) ---------------------------
NORM_MAX_WIDTH = 8192                           # the widest row the kernels take


def norm_plan(width: int) -> Tuple[int, int]:
    """(lanes per row, blocks of 8 elements per lane) of the forward kernel at ``width``: the thresholds of ``plan_of`` in fewbit_norm.hip, restated
    for the tests that stand on both sides of each.  256 / lanes rows share a forward workgroup, at most 16384 of which are launched; beyond
    that a workgroup walks on by the width of the grid.  Backward has the same thresholds: its workgroups have 1024 lanes, one block per lane
    (512 lanes per row beyond 2048 elements, 1024 beyond 4096), and there are at most 512 of them."""
    for limit, plan in ((64, (8, 1)), (128, (16, 1)), (512, (64, 1)), (1024, (128, 1)), (2048, (256, 1)), (4096, (256, 2))):
        if width <= limit:
            return plan
    return 256, 4


def norm_state_bytes(rows: int, width: int, bits: int) -> int:
    """Bytes of the state of a ``rows x width`` layer norm at ``bits`` bits: ``rows * (8 * ceil(width / 64) + C)`` with ``C = bits * ceil(width / 8)``
    rounded up to a multiple of 4; 0 for ``bits`` other than 2, 4, 8, a width outside 1 .. 8192, no rows and ``rows * width`` beyond 2^36."""
    if rows < 0 or width < 0:
        return 0
    return lib().fewbit_hipx_norm_state_bytes(rows, width, bits)


def norm_workspace_bytes(rows: int, width: int) -> int:
    """bytes of scratch ``layer_norm_backward`` needs for ``dgamma`` / ``dbeta`` and ``rms_norm_backward`` for ``dgamma`` (0: no kernel for this shape)"""
    if rows < 0 or width < 0:
        return 0
    return lib().fewbit_hipx_norm_workspace(rows, width)


_NORM = (norm_state_bytes, f'no state for {{}} rows of {{}} elements (widths 1 .. {NORM_MAX_WIDTH}, rows * width <= 2^36)')


def norm_state_host(xhat: torch.Tensor, seed: int, bits: int) -> torch.Tensor:
    """The state ``layer_norm_forward`` writes for ``seed``, evaluated on the host from given normalized rows ``xhat`` (2-D, taken as contiguous
    fp32): a host uint8 tensor of ``norm_state_bytes`` bytes.  The definition is include/fewbit_hipx.h's ("the normalized rows of a seed"): the
    packed form of a seed with groups and blocks per row; for a width that is a multiple of 64, ``quant_pack_host(xhat.flatten(), seed, bits)``."""
    if xhat.dim() != 2:
        raise FewbitHipError(f'xhat must be 2-D (got {xhat.dim()} dimensions)')
    x = xhat.detach().to(device='cpu', dtype=torch.float32).contiguous()
    rows, width = x.shape
    if rows and not 1 <= width <= NORM_MAX_WIDTH:
        _check(lib().fewbit_hipx_norm_state_host(None, rows, width, bits, 0, None))        # (the library words the refusal)
    out = torch.empty(_size(_NORM, 'norm_state_host', bits, rows, width), dtype=torch.uint8)
    _check(lib().fewbit_hipx_norm_state_host(x.data_ptr(), rows, width, bits, seed & 0xffffffffffffffff, out.data_ptr()))
    return out


def norm_state_unpack_host(state: torch.Tensor, rows: int, width: int, bits: int) -> torch.Tensor:
    """The fp32 decode of a state on the host: a float32 tensor ``rows x width`` (``fma(code, step, lo)``; a poisoned group: NaN)"""
    _state_to_read(state, _size(_NORM, 'norm_state_unpack_host', bits, rows, width), host=True)
    out = torch.empty((rows, width), dtype=torch.float32)
    _check(lib().fewbit_hipx_norm_state_unpack_host(state.data_ptr(), rows, width, bits, out.data_ptr()))
    return out


def _norm_rows(t: torch.Tensor, what: str) -> Tuple[int, int]:
    if t.device.type != 'cuda':
        raise FewbitHipError(f'{what} must live on the GPU (got {t.device})')
    if t.dtype not in DTYPES:
        raise FewbitHipError(f'unsupported dtype {t.dtype}')
    if t.dim() != 2 or not t.is_contiguous():
        raise FewbitHipError(f'{what} must be a contiguous 2-D tensor')
    return t.shape


def _norm_vector(t: Optional[torch.Tensor], like: torch.Tensor, what: str) -> Optional[int]:
    if t is None:
        return None
    if t.dtype != like.dtype or t.numel() != like.shape[1] or not t.is_contiguous():
        raise FewbitHipError(f'{what} must be a contiguous tensor of {like.shape[1]} elements of {like.dtype}')
    return t.data_ptr()


def _norm_out(t: Optional[torch.Tensor], shape, dtype: torch.dtype, device, what: str) -> torch.Tensor:
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise FewbitHipError(f'{what} must be a contiguous {" x ".join(map(str, shape))} tensor of {dtype}')
    return t


def _like(t: Optional[torch.Tensor], x: torch.Tensor, what: str) -> Optional[torch.Tensor]:
    if t is not None and (t.dtype != x.dtype or t.shape != x.shape or not t.is_contiguous()):
        raise FewbitHipError(f'{what} must be a contiguous tensor of the shape and dtype of {"x" if what in ("residual", "h") else "gy"}')
    return t


def _norm_forward(centred: bool, x, gamma, beta, eps, bits, seed, keep, want_xhat, y, rstd, state, xhat, stream, add=None):
    """The forward call of either norm -> ``(y, h, rstd, state, xhat)``: ``centred`` is the layer norm, whose entry point alone takes ``beta`` (None for
    the RMS norm).  ``add``: None, or ``(residual, p, want_h, h)`` for the entry point with ``residual + dropout(x)`` fused in front, which alone
    evaluates a threshold, needs the seed for its mask too, and writes ``h``."""
    residual, p, want_h, h = add or (None, None, False, None)
    rows, width = _norm_rows(x, 'x')
    if add is not None:
        _like(residual, x, 'residual')
    gp = _norm_vector(gamma, x, 'gamma')
    pointers = (gp, _norm_vector(beta, x, 'beta')) if centred else (gp, )
    threshold = 0 if add is None else dropout_threshold(p)
    name = ('layer_norm_forward' if centred else 'rms_norm_forward') if add is None else ('add_layer_norm_forward' if centred else 'add_rms_norm_forward')
    need = _size(_NORM, name, bits, rows, width) if keep else 0
    value, word, others = _seed_arguments(seed) if keep or threshold else (0, None, ())
    with _on(x.device):
        y = _norm_out(y, (rows, width), x.dtype, x.device, 'y')
        rstd = _norm_out(rstd, (rows, ), torch.float32, x.device, 'rstd')
        if want_h or h is not None:
            h = _norm_out(h, (rows, width), x.dtype, x.device, 'h')
        state = _state_to_write(state, keep, need, x.device)
        if want_xhat or xhat is not None:
            xhat = _norm_out(xhat, (rows, width), torch.float32, x.device, 'xhat')
        # (what the fused entry point takes besides: the residual behind x, the threshold and h around y)
        read = (x.data_ptr(), ) if add is None else (x.data_ptr(), residual.data_ptr())
        written = (y.data_ptr(), ) if add is None else (threshold, y.data_ptr(), _ptr(h))
        _same_device(x, *(() if add is None else (residual, )), y, rstd, *others, *(t for t in (gamma, beta, h, state, xhat) if t is not None))
        _check(getattr(lib(), 'fewbit_hipx_' + name)(DTYPES[x.dtype], *read, rows, width, *pointers, float(eps), bits, value, word, *written, rstd.data_ptr(),
                                                     None if state is None else state.data_ptr(), 0 if state is None else state.numel(),
                                                     None if xhat is None else xhat.data_ptr(), _stream(stream, x.device)))
    return y, h, rstd, state, xhat


def _norm_backward(centred: bool, gy, state, rstd, gamma, bits, want, outs, workspace, stream, add=None):
    """The backward call of either norm: ``want`` and ``outs`` are (dx, dgamma, dbeta) for the layer norm (``centred``) and (dx, dgamma) for the RMS norm.
    ``add``: None, or ``(gh, seed, p)`` for the backward of the fused entry point, where (dres, dbranch) stand in the place of dx and ``want`` may be
    None: everything, ``dbranch`` only with a mask."""
    gh, seed, p = add or (None, 0, None)
    rows, width = _norm_rows(gy, 'gy')
    if gh is not None:
        _like(gh, gy, 'gh')
    gp = _norm_vector(gamma, gy, 'gamma')
    threshold = 0 if add is None else dropout_threshold(p)
    if want is None:
        want = (True, threshold > 0, True, True)[:4 if centred else 3]
    name = ('layer_norm_backward' if centred else 'rms_norm_backward') if add is None else ('add_layer_norm_backward' if centred else 'add_rms_norm_backward')
    _state_to_read(state, _size(_NORM, name, bits, rows, width))
    if rstd.dtype != torch.float32 or rstd.numel() != rows or not rstd.is_contiguous():
        raise FewbitHipError(f'rstd must be a contiguous float32 tensor of {rows} elements')
    value, word, others = _seed_arguments(seed) if threshold else (0, None, ())
    with _on(gy.device):
        matrix, sums = ((rows, width), gy.dtype), (((width, ), torch.float32, 'dgamma'), ((width, ), torch.float32, 'dbeta'))
        shapes = ((*matrix, 'dx'), *sums) if add is None else ((*matrix, 'dres'), (*matrix, 'dbranch'), *sums)
        outs = tuple(_norm_out(t, shape, dtype, gy.device, what) if wanted else None for t, wanted, (shape, dtype, what) in zip(outs, want, shapes))
        if any(want[1 if add is None else 2:]) and workspace is None:
            workspace = torch.empty(norm_workspace_bytes(rows, width), dtype=torch.uint8, device=gy.device)
        _same_device(gy, state, rstd, *others, *(t for t in (gh, gamma, *outs, workspace) if t is not None))
        # (what the fused entry point takes besides: gh behind gy, the seed and the threshold behind bits)
        read = (gy.data_ptr(), ) if add is None else (gy.data_ptr(), _ptr(gh))
        mask = () if add is None else (value, word, threshold)
        _check(getattr(lib(), 'fewbit_hipx_' + name)(DTYPES[gy.dtype], *read, state.data_ptr(), rstd.data_ptr(), gp, rows, width, bits, *mask, *map(_ptr, outs),
                                                     _ptr(workspace), 0 if workspace is None else workspace.numel(), _stream(stream, gy.device)))
    return outs


def layer_norm_forward(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float, bits: int = 4, seed=0, keep: bool = True,
                       want_xhat: bool = False, y: Optional[torch.Tensor] = None, rstd: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None,
                       xhat: Optional[torch.Tensor] = None, stream: Optional[int] = None):
    """The layer norm of the rows of ``x`` (contiguous, 2-D, fp32 / fp16 / bf16, on the GPU; ``gamma`` / ``beta``: its dtype, or None) in ONE
    launch -> ``(y, rstd, state, xhat)``: ``y`` in the dtype of ``x``; ``rstd`` one fp32 per row; ``state`` the normalized rows in ``bits`` bits
    rounded with ``seed`` (a uint8 tensor of ``norm_state_bytes`` bytes; ``norm_state_host`` gives the same bytes from ``xhat``); ``xhat`` the
    fp32 normalized rows the kernel quantized, only with ``want_xhat`` (else None).  ``keep=False``: the plain forward, ``state`` is None and
    nothing but ``y`` and ``rstd`` is written -- the same bytes as with a state.  ``seed``: an int, or a one-element int64 tensor on the device
    of ``x`` that is read when the kernel runs (``cabi.next_sketch_seed``).  ``y``, ``rstd``, ``state``, ``xhat``: buffers to write into."""
    y, _, rstd, state, xhat = _norm_forward(True, x, gamma, beta, eps, bits, seed, keep, want_xhat, y, rstd, state, xhat, stream)
    return y, rstd, state, xhat


def layer_norm_backward(gy: torch.Tensor, state: torch.Tensor, rstd: torch.Tensor, gamma: Optional[torch.Tensor], bits: int, want=(True, True, True),
                        dx: Optional[torch.Tensor] = None, dgamma: Optional[torch.Tensor] = None, dbeta: Optional[torch.Tensor] = None,
                        workspace: Optional[torch.Tensor] = None, stream: Optional[int] = None):
    """The gradients of a layer norm from its state (``layer_norm_forward``) and ``gy`` (contiguous, 2-D, fp32 / fp16 / bf16; ``gamma``: its dtype,
    or None) -> ``(dx, dgamma, dbeta)``: ``dx`` in the dtype of ``gy``, ``dgamma`` and ``dbeta`` as fp32 of ``width`` elements; where ``want`` is
    False the output is None and nothing of it is computed or written.  Two launches (one when neither sum is wanted), fp32 arithmetic, a fixed
    order of every sum: the same arguments give the same bits.  ``workspace``: a uint8 tensor of ``norm_workspace_bytes(rows, width)`` bytes."""
    want_dx, want_dgamma, want_dbeta = want
    return _norm_backward(True, gy, state, rstd, gamma, bits, (want_dx, want_dgamma, want_dbeta), (dx, dgamma, dbeta), workspace, stream)


def rms_norm_forward(x: torch.Tensor, gamma: Optional[torch.Tensor], eps: float, bits: int = 4, seed=0, keep: bool = True, want_xhat: bool = False,
                     y: Optional[torch.Tensor] = None, rstd: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None,
                     xhat: Optional[torch.Tensor] = None, stream: Optional[int] = None):
    """The RMS norm of the rows of ``x`` in ONE launch -> ``(y, rstd, state, xhat)``, everything as in ``layer_norm_forward`` without ``beta``:
    ``rstd = 1 / sqrt(mean(x^2) + eps)``, ``xhat = x * rstd``, ``y = xhat * gamma`` rounded once, ``state`` the state of these ``xhat``
    (``norm_state_bytes`` bytes; ``norm_state_host`` gives the same bytes from ``xhat``).  ``eps`` is a number (``F.rms_norm``'s default
    is ``torch.finfo(x.dtype).eps``)."""
    y, _, rstd, state, xhat = _norm_forward(False, x, gamma, None, eps, bits, seed, keep, want_xhat, y, rstd, state, xhat, stream)
    return y, rstd, state, xhat


def rms_norm_backward(gy: torch.Tensor, state: torch.Tensor, rstd: torch.Tensor, gamma: Optional[torch.Tensor], bits: int, want=(True, True),
                      dx: Optional[torch.Tensor] = None, dgamma: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                      stream: Optional[int] = None):
    """The gradients of an RMS norm from its state (``rms_norm_forward``) and ``gy`` -> ``(dx, dgamma)``, everything as in ``layer_norm_backward``
    without the mean term and without ``dbeta``: ``dx = rstd * (g^ - x^q * mean(g^ * x^q))``, ``dgamma = sum_r gy * x^q``.  Two launches (one when
    ``dgamma`` is not wanted, and then no workspace); ``workspace``: a uint8 tensor of ``norm_workspace_bytes(rows, width)`` bytes."""
    want_dx, want_dgamma = want
    return _norm_backward(False, gy, state, rstd, gamma, bits, (want_dx, want_dgamma), (dx, dgamma), workspace, stream)


# ---- residual + dropout(x) fused in front of either norm (include/fewbit_hipx.h, "The sum of a seed in front of the norm") ------------------------------
def add_layer_norm_forward(x: torch.Tensor, residual: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float, p: float = 0.0,
                           bits: int = 4, seed=0, keep: bool = True, want_h: bool = False, want_xhat: bool = False, y: Optional[torch.Tensor] = None,
                           h: Optional[torch.Tensor] = None, rstd: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None,
                           xhat: Optional[torch.Tensor] = None, stream: Optional[int] = None):
    """``layer_norm_forward(dropout_apply(x, seed, p, addend=residual), gamma, beta, eps, bits, seed, keep)`` in ONE launch, bit for bit ->
    ``(y, h, rstd, state, xhat)``: ``h`` is the rounded sum ``residual + dropout(x)`` the rows of which are normalized, written only with ``want_h``
    (or a buffer ``h``), else None -- it is then never in memory.  ONE ``seed`` (an int, or a device word) gives the mask and the rounding.
    ``p``: the drop probability (``dropout_threshold``; below 1).  With a mask (threshold > 0) the width must be a multiple of 8: anything else
    is refused -- compose the two calls; without one every width 1 .. 8192 is served.  No output may overlap an input."""
    return _norm_forward(True, x, gamma, beta, eps, bits, seed, keep, want_xhat, y, rstd, state, xhat, stream, (residual, p, want_h, h))


def add_layer_norm_backward(gy: torch.Tensor, state: torch.Tensor, rstd: torch.Tensor, gamma: Optional[torch.Tensor], bits: int, seed=0, p: float = 0.0,
                            gh: Optional[torch.Tensor] = None, want=None, dres: Optional[torch.Tensor] = None, dbranch: Optional[torch.Tensor] = None,
                            dgamma: Optional[torch.Tensor] = None, dbeta: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                            stream: Optional[int] = None):
    """The gradients of ``add_layer_norm_forward`` from its state -> ``(dres, dbranch, dgamma, dbeta)``: ``dres``, the residual's, is the plain
    backward's fp32 ``dx`` plus ``gh`` (the gradient arriving at ``h``, or None) rounded ONCE; ``dbranch``, the input's, is
    ``dropout_apply(dres, seed, p)``; ``dgamma`` / ``dbeta`` are ``layer_norm_backward``'s.  ``want``: which of the four (default: all; ``dbranch``
    only with a mask -- without one it is ``dres``, and asking for it is refused).  Two launches, one when neither sum is wanted."""
    return _norm_backward(True, gy, state, rstd, gamma, bits, want, (dres, dbranch, dgamma, dbeta), workspace, stream, (gh, seed, p))


def add_rms_norm_forward(x: torch.Tensor, residual: torch.Tensor, gamma: Optional[torch.Tensor], eps: float, p: float = 0.0, bits: int = 4, seed=0,
                         keep: bool = True, want_h: bool = False, want_xhat: bool = False, y: Optional[torch.Tensor] = None, h: Optional[torch.Tensor] = None,
                         rstd: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None, xhat: Optional[torch.Tensor] = None,
                         stream: Optional[int] = None):
    """``add_layer_norm_forward`` for the RMS norm (no ``beta``): ``rms_norm_forward`` of ``residual + dropout(x)`` in ONE launch, bit for bit"""
    return _norm_forward(False, x, gamma, None, eps, bits, seed, keep, want_xhat, y, rstd, state, xhat, stream, (residual, p, want_h, h))


def add_rms_norm_backward(gy: torch.Tensor, state: torch.Tensor, rstd: torch.Tensor, gamma: Optional[torch.Tensor], bits: int, seed=0, p: float = 0.0,
                          gh: Optional[torch.Tensor] = None, want=None, dres: Optional[torch.Tensor] = None, dbranch: Optional[torch.Tensor] = None,
                          dgamma: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, stream: Optional[int] = None):
    """``add_layer_norm_backward`` for the RMS norm -> ``(dres, dbranch, dgamma)``"""
    return _norm_backward(False, gy, state, rstd, gamma, bits, want, (dres, dbranch, dgamma), workspace, stream, (gh, seed, p))


# ---- the product of a gated MLP that keeps its gate and its up in 2, 4 or 8 bits (fewbit_amd/csrc/fewbit_glu.hip) -------------------------------------
GLU_ACTIVATIONS = ('silu', 'gelu')              # gelu: the erf form


def glu_state_bytes(n: int, bits: int) -> int:
    """Bytes of the state of ``n`` elements of gate and of up at ``bits`` bits: two parts of ``quant_bytes(n, bits)`` rounded up to a multiple of 8
    each; 0 for ``bits`` other than 2, 4, 8 and for ``n`` outside 1 .. 2^36.  Evaluated on the host; no GPU needed."""
    if n < 0:
        return 0
    return lib().fewbit_hipx_glu_state_bytes(n, bits)


_GLU = (glu_state_bytes, 'no state for {} elements (1 .. 2^36 are supported)')


def _glu_activation(activation: str) -> int:
    if activation not in GLU_ACTIVATIONS:
        raise FewbitHipError(f"activation must be 'silu' or 'gelu' (got {activation!r})")
    return CONTINUOUS.index(activation)             # enum fewbit_function


def glu_state_host(gate: torch.Tensor, up: torch.Tensor, seed: int, bits: int) -> torch.Tensor:
    """The state ``glu_forward`` writes for ``seed``, evaluated on the host: ``gate`` and ``up`` (one shape; taken as contiguous fp32, so pass the
    values of a 16-bit tensor as ``.float()``) -> a host uint8 tensor of ``glu_state_bytes`` bytes.  The definition is include/fewbit_hipx.h's
    ("the gate and the up of a seed"): the first half is ``quant_pack_host(gate, seed, bits)`` filled up with zero bytes, the second half the
    same of ``up`` with the next rounding domain; ``quant_unpack_host`` decodes either half.  No GPU needed."""
    if gate.shape != up.shape:
        raise FewbitHipError(f'gate and up must have one shape (got {tuple(gate.shape)} and {tuple(up.shape)})')
    g = gate.detach().to(device='cpu', dtype=torch.float32).contiguous()
    u = up.detach().to(device='cpu', dtype=torch.float32).contiguous()
    out = torch.empty(_size(_GLU, 'glu_state_host', bits, g.numel()), dtype=torch.uint8)
    _check(lib().fewbit_hipx_glu_state_host(g.data_ptr(), u.data_ptr(), g.numel(), bits, seed & 0xffffffffffffffff, out.data_ptr()))
    return out


def _glu_rows(t: torch.Tensor, what: str) -> Tuple[int, int, int]:
    """(rows, width, row stride) of a 2-D GPU tensor with unit stride along its width and rows at least a width apart"""
    if t.device.type != 'cuda':
        raise FewbitHipError(f'{what} must live on the GPU (got {t.device})')
    if t.dtype not in DTYPES:
        raise FewbitHipError(f'unsupported dtype {t.dtype}')
    if t.dim() != 2:
        raise FewbitHipError(f'{what} must be 2-D (got {t.dim()} dimensions)')
    rows, width = t.shape
    ld = t.stride(0) if rows > 1 else width
    if (width > 1 and t.stride(1) != 1) or ld < width:
        raise FewbitHipError(f'{what} must have unit stride along its width and rows at least a width apart (strides {tuple(t.stride())})')
    return rows, width, ld


def glu_forward(gate: torch.Tensor, up: torch.Tensor, activation: str = 'silu', bits: int = 4, seed=0, keep: bool = True, y: Optional[torch.Tensor] = None,
                state: Optional[torch.Tensor] = None, stream: Optional[int] = None):
    """``act(gate) * up`` in ONE launch -> ``(y, state)``.  ``gate`` and ``up``: 2-D fp32 / fp16 / bf16 GPU tensors of one shape and dtype with
    unit stride along the width and any row stride (the halves of ``x.chunk(2, -1)`` as they are); ``y``: contiguous, their dtype, ``act`` in
    fp32 and ONE product rounded once; ``state``: both inputs in ``bits`` bits rounded with ``seed`` (a uint8 tensor of ``glu_state_bytes`` bytes;
    ``glu_state_host`` gives the same bytes).  ``keep=False``: the plain forward, ``state`` is None and ``y`` has the same bytes.  ``seed``: an int,
    or a one-element int64 tensor on the device of ``gate`` that is read when the kernel runs (``cabi.next_sketch_seed``).  ``y``, ``state``:
    buffers to write into."""
    rows, width, ld_gate = _glu_rows(gate, 'gate')
    if up.shape != gate.shape or up.dtype != gate.dtype:
        raise FewbitHipError('up must have the shape and dtype of gate')
    ld_up = _glu_rows(up, 'up')[2]
    act = _glu_activation(activation)
    need = _size(_GLU, 'glu_forward', bits, rows * width) if keep else 0
    value, word, others = _seed_arguments(seed) if keep else (0, None, ())
    with _on(gate.device):
        y = _norm_out(y, (rows, width), gate.dtype, gate.device, 'y')
        state = _state_to_write(state, keep, need, gate.device)
        _same_device(gate, up, y, *others, *(() if state is None else (state, )))
        _check(lib().fewbit_hipx_glu_forward(DTYPES[gate.dtype], act, gate.data_ptr(), ld_gate, up.data_ptr(), ld_up, rows, width, bits, value, word, y.data_ptr(),
                                             _ptr(state), 0 if state is None else state.numel(), _stream(stream, gate.device)))
    return y, state


def _glu_backward(name: str, gy: Optional[torch.Tensor], like: torch.Tensor, state, activation: str, bits: int, outputs, stream, act: Optional[int] = None):
    """What the two backward entry points share, behind what each refuses first: ``like`` carries the shape and the dtype (``gy``, or the product buffer
    where there is no ``gy``); ``outputs``: (buffer or None, wanted, name) of every output the entry point ``name`` writes, in its order; ``act``: the
    activation where the caller has evaluated it already"""
    if gy is not None and (gy.dim() != 2 or not gy.is_contiguous()):
        raise FewbitHipError('gy must be a contiguous 2-D tensor')
    rows, width, _ = _glu_rows(like, 'product' if gy is None else 'gy')
    if act is None:
        act = _glu_activation(activation)
    _state_to_read(state, _size(_GLU, name, bits, rows * width))
    with _on(like.device):
        outs, written = [], []                                  # (written: pointer and row stride of every output, as the entry point takes them)
        for t, wanted, what in outputs:
            if not wanted:
                t = None
            elif t is None:
                t = torch.empty((rows, width), dtype=like.dtype, device=like.device)
            elif t.dtype != like.dtype or tuple(t.shape) != (rows, width):
                raise FewbitHipError(f'{what} must be a {rows} x {width} tensor of {like.dtype}')
            outs.append(t)
            written += (None, 0) if t is None else (t.data_ptr(), _glu_rows(t, what)[2])
        _same_device(like, state, *(t for t in outs if t is not None))
        _check(getattr(lib(), f'fewbit_hipx_{name}')(DTYPES[like.dtype], act, _ptr(gy), state.data_ptr(), rows, width, bits,
                                                     *written, _stream(stream, like.device)))
    return tuple(outs)


def glu_backward(gy: torch.Tensor, state: torch.Tensor, activation: str, bits: int, want=(True, True), d_gate: Optional[torch.Tensor] = None,
                 d_up: Optional[torch.Tensor] = None, stream: Optional[int] = None):
    """The gradients of ``act(gate) * up`` from its state (``glu_forward``) and ``gy`` (contiguous, 2-D, fp32 / fp16 / bf16) in ONE launch ->
    ``(d_gate, d_up)`` in the dtype of ``gy``: ``d_up = gy * act(g^)``, ``d_gate = (gy * u^) * act'(g^)`` on the decodes, fp32, rounded once.  Where
    ``want`` is False the output is None and nothing of it is computed or written.  ``d_gate``, ``d_up``: buffers to write into, 2-D of the
    shape of ``gy`` with unit stride along the width and any row stride -- the halves of ONE ``rows x 2 width`` tensor, for a packed
    ``[gate | up]`` input; the gap of a row stride is not written."""
    return _glu_backward('glu_backward', gy, gy, state, activation, bits, ((d_gate, want[0], 'd_gate'), (d_up, want[1], 'd_up')), stream)


def glu_backward_product(gy: Optional[torch.Tensor], state: torch.Tensor, activation: str, bits: int, want=(True, True, True), d_gate: Optional[torch.Tensor] = None,
                         d_up: Optional[torch.Tensor] = None, product: Optional[torch.Tensor] = None, stream: Optional[int] = None):
    """``glu_backward`` that also rebuilds the product from the state, in the same ONE launch -> ``(d_gate, d_up, product)`` in the dtype of ``gy``:
    ``d_gate`` and ``d_up`` with the bytes of ``glu_backward``, ``product = act(g^) * u^``, the forward's own expression on the decodes (``act`` in
    fp32, one product, rounded once) -- what a ``down_proj`` behind the product needs for its weight gradient, so that nothing of ``y`` is kept.
    Where ``want`` is False the output is None and nothing of it is computed or written; nothing wanted: no launch.  ``gy`` may be None when
    neither gradient is wanted: the shape and the dtype are then those of ``product``, which must be given.  ``d_gate``, ``d_up``, ``product``:
    buffers to write into, 2-D of the shape of ``gy`` with unit stride along the width and any row stride; the gap of a row stride is not
    written.  A poisoned group is NaN on its 64 elements of all three outputs."""
    want = tuple(bool(w) for w in want)
    if len(want) != 3:
        raise FewbitHipError('want must name three outputs (d_gate, d_up, product)')
    # (what needs no look at a tensor is refused first)
    act = _glu_activation(activation)
    if bits not in QUANT_BITS:
        raise FewbitHipError(f'glu_backward_product: bits must be 2, 4 or 8 (got {bits})')
    if gy is None:
        if want[0] or want[1]:
            raise FewbitHipError('gy may be None only when neither d_gate nor d_up is wanted')
        if not want[2]:
            return None, None, None
        if product is None:
            raise FewbitHipError('without gy the product buffer must be given: it carries the shape and the dtype')
    outputs = ((d_gate, want[0], 'd_gate'), (d_up, want[1], 'd_up'), (product, want[2], 'product'))
    return _glu_backward('glu_backward_product', gy, product if gy is None else gy, state, activation, bits, outputs, stream, act)


# ---- the cross entropy of a row that keeps the logits as given and one float per row (fewbit_amd/csrc/fewbit_xent.hip) -----------------------------------
CROSS_ENTROPY_MAX_GROUPS = 2048                 # workgroups of either launch (kMaxGroups in fewbit_xent.hip), one row each at a time; beyond it they walk on


def cross_entropy_host(logits: torch.Tensor, target: torch.Tensor, ignore_index: int = -100, grow: Optional[torch.Tensor] = None, want_grad: bool = True):
    """The definition (include/fewbit_hipx.h, "The loss of a row") evaluated on the host in float64 -> ``(lse, loss, dlogits)``: ``logits`` 2-D (taken
    as contiguous fp32, so pass the values of a 16-bit tensor as ``.float()``), ``target`` int64 of ``rows`` elements, ``grow`` one number per row (or
    None: 1).  ``lse`` and ``loss``: float64 of ``rows`` elements; ``dlogits``: float64 ``rows x width``, or None without ``want_grad``.  No GPU needed."""
    if logits.dim() != 2:
        raise FewbitHipError(f'logits must be 2-D (got {logits.dim()} dimensions)')
    x = logits.detach().to(device='cpu', dtype=torch.float32).contiguous()
    rows, width = x.shape
    t = target.detach().to(device='cpu', dtype=torch.int64).contiguous()
    if t.numel() != rows:
        raise FewbitHipError(f'target must have {rows} elements (got {t.numel()})')
    g = None if grow is None else grow.detach().to(device='cpu', dtype=torch.float64).expand(rows).contiguous()
    lse, loss = torch.empty(rows, dtype=torch.float64), torch.empty(rows, dtype=torch.float64)
    dlogits = torch.empty((rows, width), dtype=torch.float64) if want_grad else None
    _check(lib().fewbit_hipx_cross_entropy_host(x.data_ptr(), t.data_ptr(), rows, width, ignore_index, _ptr(g), lse.data_ptr(), loss.data_ptr(), _ptr(dlogits)))
    return lse, loss, dlogits


def _logits_rows(t: torch.Tensor, what: str) -> Tuple[int, int, int]:
    """(rows, width, row stride) of a 2-D GPU tensor of logits: unit stride along the width, rows at least a width apart"""
    if t.device.type != 'cuda':
        raise FewbitHipError(f'{what} must live on the GPU (got {t.device})')
    if t.dtype not in DTYPES:
        raise FewbitHipError(f'unsupported dtype {t.dtype}')
    if t.dim() != 2:
        raise FewbitHipError(f'{what} must be 2-D (got {t.dim()} dimensions)')
    rows, width = t.shape
    ld = t.stride(0) if rows > 1 else width
    if (width > 1 and t.stride(1) != 1) or ld < width:
        raise FewbitHipError(f'{what} must have unit stride along its width and rows at least a width apart (strides {tuple(t.stride())})')
    return rows, width, ld


def _row_vector(t: Optional[torch.Tensor], dtype: torch.dtype, rows: int, device, what: str) -> torch.Tensor:
    if t is None:
        return torch.empty(rows, dtype=dtype, device=device)
    if t.dtype != dtype or t.numel() != rows or not t.is_contiguous():
        raise FewbitHipError(f'{what} must be a contiguous {dtype} tensor of {rows} elements')
    return t


def cross_entropy_forward(logits: torch.Tensor, target: torch.Tensor, ignore_index: int = -100, lse: Optional[torch.Tensor] = None,
                          loss: Optional[torch.Tensor] = None, stream: Optional[int] = None):
    """``(lse, loss)`` of the rows of ``logits`` in ONE launch: ``lse = logsumexp(logits.float(), 1)`` and ``loss = F.cross_entropy(logits.float(),
    target, reduction='none', ignore_index=ignore_index)`` as float32 tensors of ``rows`` elements, each row read once.  ``logits``: a 2-D fp32 / fp16 /
    bf16 GPU tensor with unit stride along the classes and any row stride and alignment (a row-sliced view as it is); ``target``: int64 of ``rows``
    elements on its device.  An ignored row has loss +0; a target outside ``[0, width)`` gives NaN (no device assertion); a row with a NaN or a
    ``+inf``, or of ``-inf`` only, gives NaN.  ``lse``, ``loss``: buffers to write into.  Enqueued on torch's current stream; nothing is read back."""
    rows, width, ld = _logits_rows(logits, 'logits')
    if target.dtype != torch.int64 or target.numel() != rows or not target.is_contiguous():
        raise FewbitHipError(f'target must be a contiguous int64 tensor of {rows} elements')
    with _on(logits.device):
        lse = _row_vector(lse, torch.float32, rows, logits.device, 'lse')
        loss = _row_vector(loss, torch.float32, rows, logits.device, 'loss')
        _same_device(logits, target, lse, loss)
        _check(lib().fewbit_hipx_cross_entropy_forward(DTYPES[logits.dtype], logits.data_ptr(), rows, width, ld, target.data_ptr(), ignore_index, lse.data_ptr(),
                                                       loss.data_ptr(), _stream(stream, logits.device)))
    return lse, loss


def cross_entropy_backward(logits: torch.Tensor, target: torch.Tensor, lse: torch.Tensor, grow: torch.Tensor, ignore_index: int = -100,
                           out: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    """``grow * (softmax(logits.float(), 1) - one_hot(target))`` rounded once to the dtype of ``logits``, in ONE launch that reads every element once
    and writes it once.  ``lse``: what ``cross_entropy_forward`` gave for these logits; ``grow``: a float32 GPU tensor of ONE element (the same
    gradient for every row: a sum, or a mean with ``1 / count`` multiplied in) or of ``rows`` elements -- a device tensor either way, nothing is read
    back.  ``out``: a 2-D tensor of the shape and dtype of ``logits`` with unit stride along the classes and any row stride; ``out is logits`` (or the
    same memory and strides) is the backward in place: the gradient replaces the logits, bit for bit.  An ignored row is +0, a row whose target is out
    of range is NaN."""
    rows, width, ld = _logits_rows(logits, 'logits')
    if target.dtype != torch.int64 or target.numel() != rows or not target.is_contiguous():
        raise FewbitHipError(f'target must be a contiguous int64 tensor of {rows} elements')
    _row_vector(lse, torch.float32, rows, logits.device, 'lse')
    if grow.dtype != torch.float32 or grow.numel() not in (1, rows) or not grow.is_contiguous():
        raise FewbitHipError(f'grow must be a contiguous float32 tensor of 1 or {rows} elements')
    with _on(logits.device):
        if out is None:
            out = torch.empty((rows, width), dtype=logits.dtype, device=logits.device)
        elif out.dtype != logits.dtype or tuple(out.shape) != (rows, width):
            raise FewbitHipError(f'out must be a {rows} x {width} tensor of {logits.dtype}')
        ld_out = _logits_rows(out, 'out')[2]
        _same_device(logits, target, lse, grow, out)
        _check(lib().fewbit_hipx_cross_entropy_backward(DTYPES[logits.dtype], logits.data_ptr(), rows, width, ld, target.data_ptr(), ignore_index, lse.data_ptr(),
                                                        grow.data_ptr(), 0 if grow.numel() == 1 else 1,
                                                        out.data_ptr(), ld_out, _stream(stream, logits.device)))
    return out
