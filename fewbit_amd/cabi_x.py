"""ctypes binding of the companion library ``libfewbit_hipx.so`` (include/fewbit_hipx.h): the entry points added after the C-ABI
of ``libfewbit_hip.so`` was frozen at version 5 (``cabi.SYMBOLS`` stays that list).  Same conventions as ``cabi``: device tensors,
torch's current stream on the tensors' device, no fallback -- a missing library or an unsupported shape raises.
"""
import ctypes
import os
from pathlib import Path
from typing import Optional

import torch

from .cabi import DTYPES, FewbitHipError, _sampled_call, _seed_word, _stream

__all__ = ['LIB_PATH', 'ABI_VERSION', 'SYMBOLS', 'lib', 'sampled_dft', 'sampled_dft_seeded', 'sampled_dft_workspace_bytes']

LIB_PATH = Path(os.environ.get('FEWBIT_HIPX_LIB') or Path(__file__).resolve().with_name('libfewbit_hipx.so'))
ABI_VERSION = 1                                # FEWBIT_HIPX_ABI_VERSION this binding was written against

# every symbol include/fewbit_hipx.h declares
SYMBOLS = ('fewbit_hipx_abi_version', 'fewbit_hipx_last_error', 'fewbit_hipx_sampled_dft_workspace', 'fewbit_hipx_sampled_dft',
           'fewbit_hipx_sampled_dft_seeded')

_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise FewbitHipError(f'{LIB_PATH} is missing: build it with `make -C fewbit_amd/csrc` '
                                 '(or `python -c "import __graft_entry__ as g; g.build()"`)')
        L = ctypes.CDLL(str(LIB_PATH))
        vp, sz, i32, dbl, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double, ctypes.c_uint64
        L.fewbit_hipx_abi_version.restype = i32
        L.fewbit_hipx_abi_version.argtypes = []
        have = L.fewbit_hipx_abi_version()
        if have < ABI_VERSION:
            raise FewbitHipError(f'{LIB_PATH} has ABI version {have}, this binding needs {ABI_VERSION}: rebuild it (make -C fewbit_amd/csrc)')
        L.fewbit_hipx_last_error.restype = ctypes.c_char_p
        L.fewbit_hipx_last_error.argtypes = []
        L.fewbit_hipx_sampled_dft_workspace.restype = sz
        L.fewbit_hipx_sampled_dft_workspace.argtypes = [i32, sz, sz, sz]
        L.fewbit_hipx_sampled_dft.restype = i32
        L.fewbit_hipx_sampled_dft.argtypes = [i32, vp, sz, sz, sz, vp, sz, dbl, i32, vp, vp, sz, vp]
        L.fewbit_hipx_sampled_dft_seeded.restype = i32
        L.fewbit_hipx_sampled_dft_seeded.argtypes = [i32, vp, sz, sz, sz, u64, vp, sz, dbl, i32, vp, vp, sz, vp]
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


def _sampled_dft_call(m: torch.Tensor, proj: int, out_dtype: Optional[torch.dtype], out: Optional[torch.Tensor], workspace: Optional[torch.Tensor],
                      others, launch) -> torch.Tensor:
    out_dtype = m.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, m.dtype):
        raise FewbitHipError(f'out_dtype must be torch.float32 or the dtype of m (got {out_dtype})')
    return _sampled_call('sampled_dft', sampled_dft_workspace_bytes, _check, m, proj, (2, ), out_dtype, '2 x proj x features tensor of out_dtype', out,
                         workspace, others, lambda dt, *rest: launch(dt, DTYPES[out_dtype], *rest))


def sampled_dft(m: torch.Tensor, idx: torch.Tensor, scale: float = 1.0, out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    """``scale * torch.fft.fft(m, dim=0, norm='ortho')[idx]`` for a 2-D ``m`` (rows x features, unit stride along the features) whose row
    count is one of ``cabi.SAMPLED_ROWS``; ``idx``: int64 row numbers on the device of ``m``.
    fp32 arithmetic.  Returns a ``(2, proj, features)`` tensor of ``out_dtype`` (torch.float32 or the dtype of ``m``, the default):
    ``[0]`` the real part, ``[1]`` the imaginary part.

    Features ``(2c, 2c + 1)`` are transformed as one complex column: the rounding error of column ``c`` scales with the RMS of the pair
    ``(c, c ^ 1)``, and a NaN or Inf in one column makes its partner non-finite too (other columns stay bit for bit as they are).
    torch.fft keeps every column apart."""
    if idx.dtype != torch.int64 or idx.dim() != 1 or idx.device != m.device or not idx.is_contiguous():
        raise FewbitHipError('idx must be a contiguous 1-D int64 tensor on the device of m')
    proj = idx.numel()
    return _sampled_dft_call(m, proj, out_dtype, out, workspace, (idx, ), lambda dt, odt, mp, rows, features, ld, op, wp, wb: lib().fewbit_hipx_sampled_dft(
        dt, mp, rows, features, ld, idx.data_ptr(), proj, scale, odt, op, wp, wb, _stream(stream, m.device)))


def sampled_dft_seeded(m: torch.Tensor, proj: int, seed, scale: float = 1.0, out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None,
                       workspace: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    """``sampled_dft(m, cabi.sampled_rows(seed, rows, proj))`` without the array of row numbers: the rows are a function of ``seed`` that the
    kernel evaluates itself (the rows ``cabi.sampled_dct_seeded`` samples).  ``seed``: an int, or a one-element int64 tensor on the device of
    ``m`` whose value is read when the kernel runs (``cabi.next_sketch_seed``: a launch recorded into a hipGraph then samples fresh rows on
    every replay).  The pair contract of ``sampled_dft`` holds: column ``c``'s error scales with the RMS of the pair ``(c, c ^ 1)``, a
    non-finite value reaches the partner."""
    if isinstance(seed, torch.Tensor):
        _seed_word(seed, 'seed')
        value, word, others = 0, seed.data_ptr(), (seed, )
    else:
        value, word, others = seed & 0xffffffffffffffff, 0, ()
    return _sampled_dft_call(m, proj, out_dtype, out, workspace, others, lambda dt, odt, mp, rows, features, ld, op, wp, wb: lib().fewbit_hipx_sampled_dft_seeded(
        dt, mp, rows, features, ld, value, word, proj, scale, odt, op, wp, wb, _stream(stream, m.device)))
