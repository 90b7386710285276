"""Linear layers that keep a *compressed* copy of their input for the weight gradient.

Counterpart of the reference's randomized layers (``fewbit/functional/linear.py``, ``fewbit/modules/linear.py``;
paper: "Memory-Efficient Backpropagation through Large Linear Layers", arXiv:2201.13195).  Same public names
(``linear_crs``, ``linear_grp``, ``linear_randomized``; ``LinearCRS``, ``LinearGRP``, ``RandomizedLinear``) and
constructor / call signatures; the implementation is this repository's own:

* forward is exactly ``F.linear``; the input gradient is exact; only ``dL/dW = G^T X`` (G, X: rows x features) is
  estimated, from a sketch ``S`` (p x rows, ``E[S^T S] = I``): saved for backward is ``S X`` (p rows instead of
  ``rows``), backward recomputes ``S`` from the saved generator state and forms ``(S G)^T (S X)``;
* the sketch is drawn in the *input's dtype*, so with bf16/fp16 activations both sketch GEMMs run on the matrix
  cores (hipBLASLt through ``torch.matmul``) -- the reference draws fp32 and cannot multiply it with 16-bit inputs;
* ``sketch_dtype`` (extension): dtype the two dense sketch products ``S X`` and ``S G`` are computed in -- and, on the
  GPU kernel, the dtype the projection is KEPT in.  ``S G`` costs four times the exact weight-gradient GEMM at ratio 0.2, so
  for fp32 layers ``sketch_dtype=torch.bfloat16`` moves those flops onto the bf16 matrix cores; with this package's kernel
  (which rounds fp32 operands to bf16 anyway) what the option adds is a bf16 projection -- half the saved bytes -- and a
  bf16 final GEMM: RoBERTa-base fp32, Rademacher, ratio 0.2: 1.01x the vanilla step at -26.4 % peak memory instead of
  1.02x at -21.5 %.  The rounding of the projections to 8 bits is zero-mean and far below the variance of the estimator;
* every sketch is unbiased.  The reference's ``'dct'``/``'dft'`` branches scale the sampled rows by ``p * rows``
  (``fewbit/functional/linear.py:124-137``) where unbiasedness needs ``rows / p``, and its ``'dft'`` backward drops
  the imaginary part before the product (:189-197, :214-216); neither defect is reproduced (they are not covered by
  the reference's tests, which only run the default ``'gaussian'``, ``fewbit/modules/linear_test.py``);
* without a user generator the sketch seed comes from the host default generator (so ``torch.manual_seed`` makes
  runs reproducible) and never reads back from the device -- no stream synchronisation in forward or backward;
* on the GPU the dense sketches (``'gaussian'``, ``'rademacher'``) of fp32 / fp16 / bf16 tensors run on this package's own
  gfx950 kernels (``fewbit_amd/csrc/fewbit_sketch.hip`` through the C-ABI ``fewbit_hip_sketch``): ``S`` is a pure function
  of a 64-bit seed (Philox4x32-10; Gaussian: xoshiro128++ streams seeded by it) -- Rademacher signs are generated in registers
  and fed straight to the matrix cores, a Gaussian ``S`` of a layer wider than 256 features is written once per product into a
  scratch workspace as MFMA fragments and read back (it costs as much to generate as to multiply: regenerating it per column
  tile was slower than ``randn`` + ``matmul``); what a layer keeps for backward is the ``p x features`` projection and ONE
  integer, and backward regenerates the same ``S`` from that integer.  The reference draws ``proj x rows`` random numbers into
  device memory twice per layer and step (fewbit/functional/linear.py:133-137,195-199).  fp32 operands are rounded to bf16 on their
  way into the matrix pipe (accumulation is fp32): a zero-mean relative perturbation of 2^-9 per element under an estimator
  whose own relative noise is ~ sqrt(rows / p).  ``use_native_sketch(False)`` (or ``FEWBIT_SKETCH_NATIVE=0``) selects
  the PyTorch formulation (randn / randint + matmul) instead, and so does an EXPLICIT ``sketch_dtype=torch.float32`` /
  ``float64`` (a request for products of that precision); host tensors and float64 always take it;
* the native path can be captured into a hipGraph (``torch.cuda.graph``) after one eager warm-up call per device: while
  the stream is capturing, the seed is a device word that a recorded one-thread kernel re-derives on every replay
  (``_sketch_seed``), so a replayed training step draws a fresh ``S`` each time -- a seed recorded by value would repeat
  one matrix for ever.  (The reference reads the generator state back in forward and cannot be captured.)
* inside training wrappers: backward runs under the autocast state its forward saw (``backward()`` may follow the ``autocast`` block); with
  grad mode off, a frozen weight or no rows the layers are ``F.linear`` and nothing else (``_plain_linear``); backward reads its saved
  tensors once (non-re-entrant checkpointing) and works on a contiguous ``grad_output`` (one gradient, one result, whatever its strides).

The sampled transforms: 'dct' and 'dft' on 2-D GPU tensors of 2^8 .. 2^18, 3 x 2^8 .. 3 x 2^14, 5 x 2^8 .. 5 x 2^13, 7 x 2^9 .. 7 x 2^13,
9 x 2^8 .. 9 x 2^12 or 15 x 2^8 .. 15 x 2^11 rows (``cabi.SAMPLED_ROWS``) run on this
package's kernel pairs (``fewbit_hip_sampled_dct``, ``fewbit_amd/csrc/fewbit_dct.hip``; ``fewbit_hipx_sampled_dft`` of the companion
library, ``fewbit_amd/csrc/fewbit_dft.hip``): one four-step fp32 FFT in LDS that writes only the sampled rows -- the torch.fft formulation
costs 110-120 x the bytes of the result, profiles/r06_sketch_bench.json.  'dft' keeps its real and imaginary parts as two planes in the
layer's dtype (two ``p x features`` views of one buffer; for a 16-bit layer half the bytes of torch.fft's complex64), and its weight
gradient ``Gr^T Xr + Gi^T Xi`` is two accumulating GEMMs in the planes' dtype.  Other shapes are PyTorch-level code.  Inside the layer the
sampled rows are, like ``S``, a function of the call's 64-bit seed that the kernel evaluates itself (``fewbit_hip_sampled_dct_seeded``,
``fewbit_hipx_sampled_dft_seeded``; ``cabi.sampled_rows(seed, rows, p)`` is the same function on the host): no ``randint`` launch, no saved
RNG state, and the layer can be captured into a hipGraph.  ``use_native_sketch(False)`` selects torch.fft + randint.  SURVEY section 8f, row 4.

Any other row count (100 or 50 sequences, the short last batch of an epoch): torch.fft by default; with ``use_row_extension(True)`` (or
``FEWBIT_EXTEND_ROWS=1``) the kernel pairs at the next supported row count N' (``cabi_x.sampled_rows_ceil``) by zero extension
(``fewbit_hipx_sampled_dct_zext_seeded`` / ``_dft_zext_seeded``: the missing rows are zeros pass A never loads, there is no padded copy).
With R sampling p of N' rows uniformly with replacement, C' the orthonormal transform of length N' and P the N' x N matrix that appends
the zero rows, S = sqrt(N' / p) R C' P has E[S^T S] = (N' / p) P^T C'^T (p / N') C' P = P^T P = I_N, so ``(S G)^T (S X)`` with the same R in
forward (scale N' / p) and backward (scale 1) is an unbiased estimate of ``G^T X``.  It is an estimator of the same kind as the layer's own
but NOT the reference's ``dct(X)[idx]`` at length N -- another random variable with the same mean -- which is why it is opt-in.

Random signs in front of the transform: with ``use_sign_flips(True)`` (or ``FEWBIT_SIGN_FLIPS=1``; off by default) 'dct' and 'dft' use
``S = sqrt(N / p) R T D`` with ``D = diag(+-1)``, the subsampled RANDOMIZED transform.  ``E[S^T S] = D T^H T D = I`` for every ``D``, so the
estimate stays unbiased; what ``D`` buys is the variance: without it a component many rows share (a mean activation, a repeated token) lands in
a few rows of ``T X`` that the ``p`` samples hit or miss, and the variance grows like ``N`` times the dense sketches' level; with it the level
``VarianceEstimator``'s ``var_rmm`` assumes holds.  On the kernel pairs the signs are, like the rows, a function of the call's seed
(``cabi_x.sampled_signs(seed, rows)`` on the host) that pass A evaluates itself and XORs into the rows it has just loaded
(``fewbit_hipx_sampled_dct_signed`` / ``_dft_signed``, zero-extended with ``use_row_extension()``): still one integer kept for backward, no
read-back, capturable after one eager call, and autocast, checkpoint and ``no_grad`` behave as above.  The PyTorch formulation draws ``D``
from the call's generator before the rows.  The autograd node records whether its forward flipped; backward follows the record.

Column sampling: ``linear_crs`` / ``LinearCRS`` on fp32 / fp16 / bf16 GPU tensors follows the same contract on the kernels of
``fewbit_amd/csrc/fewbit_crs.hip`` (companion library: ``fewbit_hipx_crs_gather``, ``fewbit_hipx_crs_scatter``): the drawn columns are a function
of the call's seed (``cabi_x.crs_columns(seed, in_features, nopairs)`` on the host), forward is one gather-and-scale call, backward one GEMM and
one call that writes the whole weight gradient; the layer keeps its ``rows x m`` projection and one integer, reads nothing back and can be
captured into a hipGraph (a captured layer keeps ``min(nopairs, in_features)`` columns, the unused ones zero).  ``use_native_sketch(False)``
selects randint + bincount + nonzero, with its read-back.

Every element in a few bits: ``linear_quantized`` / ``QuantizedLinear`` (this package's own; like ``Dropout`` they are not in
``fewbit.modules.__all__``, which stays the reference's list) keep the WHOLE input, each element rounded to ``bits`` = 2, 4 or 8 bits --
the other standard way to shrink what a linear layer saves, for users who cannot afford the variance of a projection that throws rows or
columns away.  Per group of 64 consecutive elements (by flat index) the minimum ``lo`` and ``step = (max - lo) / (2^bits - 1)`` are kept as
fp32 and every element as ``code = min(L, floor((x - lo) / step + U))`` with ``U`` uniform in [0, 1): ``E[lo + code * step] = x``, the error
of an element is below ``step``, a constant group is exact.  Forward is ``F.linear``; ``grad_input`` and ``grad_bias`` are exact;
``grad_weight = G^T X^`` with ``X^`` decoded into the gradient's dtype as a transient tensor -- one GEMM (a bf16 gradient at 8 bits: X^ decoded
into fp32 and multiplied as two bf16 terms that meet in fp32, ``kept.decode_in_two_terms``: about twice the time of the other widths).  On fp32 / fp16 / bf16 GPU tensors
packing and decoding are one launch each on the kernels of ``fewbit_amd/csrc/fewbit_quant.hip`` (``cabi_x.quant_pack`` / ``quant_unpack``;
the definition, "the packed form of a seed", is include/fewbit_hipx.h's and ``cabi_x.quant_pack_host`` evaluates it on the host): ``U`` is a
function of the call's 64-bit seed, the node keeps one uint8 buffer of ``cabi_x.quant_bytes(input.numel(), bits)`` bytes (0.3125 x a bf16
input at 4 bits, 0.1875 x at 2, 0.5625 x at 8), the weight, the seed and the shape -- never the input -- reads nothing back and can be
captured into a hipGraph after one eager call (the seed is then a device word: every replay rounds afresh).  A group that holds a NaN or an
infinity decodes to NaN as a whole; other groups are untouched.  Host tensors, float64 and ``use_native_sketch(False)`` take a PyTorch
formulation of the same scheme (the same groups, the same unbiased rounding, ``U`` from the call's generator, one code per byte; not bit
for bit the kernel's).  Autocast, checkpointing, ``no_grad`` and a frozen weight behave as for the layers above.  Out of scope: fusing the
decode into the GEMM, 3-bit codes, per-row groups.
"""
import contextlib
import os
from typing import Optional

import torch
import torch.nn.functional as F

from .fft import dct

__all__ = ('MATMUL_TYPES', 'projection_dim', 'linear_crs', 'linear_grp', 'linear_randomized', 'LinearCRS', 'LinearGRP',
           'RandomizedLinear', 'use_native_sketch', 'use_row_extension', 'use_sign_flips', 'sampled_transform', 'sampled_transform_path',
           'QUANT_BITS', 'linear_quantized', 'QuantizedLinear')

MATMUL_TYPES = ('dct', 'dft', 'gaussian', 'rademacher')


def projection_dim(rows: int, proj_dim_ratio: Optional[float] = None, proj_dim: Optional[int] = None,
                   proj_dim_max: Optional[int] = None, proj_dim_min: Optional[int] = None) -> int:
    """Number of sketch rows for an input of ``rows`` rows: ``proj_dim``, else ``int(ratio * rows)``, clamped to
    ``[proj_dim_min, proj_dim_max]`` (reference: ``LinearGRPFunc.calc_proj_dim``, fewbit/functional/linear.py:73-83)."""
    if proj_dim:
        p = int(proj_dim)
    elif proj_dim_ratio:
        p = int(proj_dim_ratio * rows)
    else:
        p = int(rows)
    if proj_dim_min:
        p = max(int(proj_dim_min), p)
    if proj_dim_max:
        p = min(int(proj_dim_max), p)
    return max(p, 1)


# ---- random state that can be replayed in backward ------------------------------------------------------------------

def _capture_rng(generator: Optional[torch.Generator], device: torch.device):
    """-> (token, generator to draw from now).  The token rebuilds an identical generator later."""
    if generator is not None:
        return ('state', generator.device, generator.get_state()), generator
    seed = int(torch.randint(0, 2**62, (), dtype=torch.int64).item())          # host generator: no device round trip
    gen_device = device if device.type == 'cuda' else torch.device('cpu')
    return ('seed', gen_device, seed), torch.Generator(device=gen_device).manual_seed(seed)


def _replay_rng(token) -> torch.Generator:
    kind, device, payload = token
    gen = torch.Generator(device=device)
    if kind == 'seed':
        gen.manual_seed(payload)
    else:
        gen.set_state(payload)
    return gen


# ---- the gfx950 kernel for the dense sketches ---------------------------------------------------------------------

_NATIVE_SKETCH = os.environ.get('FEWBIT_SKETCH_NATIVE', '1') not in ('0', 'no', 'false')


def use_native_sketch(on: Optional[bool] = None) -> bool:
    """Query / set whether GPU tensors take this package's kernels -- the Philox-in-register MFMA kernel for 'gaussian' /
    'rademacher' sketches, the sampled-transform kernel pairs for 'dct' and 'dft', the column-sampling kernels of ``linear_crs`` / ``LinearCRS``
    (default) -- or the PyTorch formulation (randn / randint + matmul, torch.fft; for ``linear_crs`` randint + bincount + nonzero, which
    reads back from the device).  Returns the previous setting."""
    global _NATIVE_SKETCH
    prev = _NATIVE_SKETCH
    if on is not None:
        _NATIVE_SKETCH = bool(on)
    return prev


_EXTEND_ROWS = os.environ.get('FEWBIT_EXTEND_ROWS', '0') in ('1', 'yes', 'true')


def use_row_extension(on: Optional[bool] = None) -> bool:
    """Query / set whether 'dct' / 'dft' on a 2-D fp32 / fp16 / bf16 GPU tensor whose row count N has no kernel run on the kernel pairs at
    the next supported count N' by zero extension (``cabi_x.sampled_*_zext_seeded``) instead of torch.fft.  Off by default (environment:
    ``FEWBIT_EXTEND_ROWS=1`` turns it on): the zero-extended estimator is unbiased (module docstring) but is not the reference's
    ``dct(X)[idx]`` at length N.  Needs ``use_native_sketch()`` on; row counts with a kernel, and those above 262144, are not affected.
    Returns the previous setting."""
    global _EXTEND_ROWS
    prev = _EXTEND_ROWS
    if on is not None:
        _EXTEND_ROWS = bool(on)
    return prev


_SIGN_FLIPS = os.environ.get('FEWBIT_SIGN_FLIPS', '0') in ('1', 'yes', 'true')


def use_sign_flips(on: Optional[bool] = None) -> bool:
    """Query / set whether 'dct' and 'dft' (``linear_grp`` / ``LinearGRP`` / ``RandomizedLinear``, ``sampled_transform``) negate a random
    half of the rows before the transform: ``S = sqrt(N / p) R T D``, ``D = diag(+-1)`` (module docstring).  Off by default (environment:
    ``FEWBIT_SIGN_FLIPS=1`` turns it on); off, nothing changes.  A backward follows what its forward did, not this switch.  Returns the
    previous setting."""
    global _SIGN_FLIPS
    prev = _SIGN_FLIPS
    if on is not None:
        _SIGN_FLIPS = bool(on)
    return prev


def _native_sketch_applies(kind: str, mat: torch.Tensor, sketch_dtype) -> bool:
    """The kernel multiplies on the 16-bit matrix pipe (fp32 input is rounded to bf16, sums are fp32).  ``sketch_dtype=None``
    (the default) and the 16-bit dtypes take it; an EXPLICIT ``sketch_dtype=torch.float32`` / ``float64`` asks for products of
    that precision and gets the PyTorch formulation (S drawn into memory, library GEMM in that dtype) instead."""
    return (_NATIVE_SKETCH and _INJECTED is None and kind in ('gaussian', 'rademacher') and mat.device.type == 'cuda'
            and mat.dtype in (torch.float32, torch.float16, torch.bfloat16) and mat.dim() == 2 and mat.shape[0] > 0
            and sketch_dtype in (None, torch.bfloat16, torch.float16))


def _mix64(a: int, b: int) -> int:
    """splitmix64 of (a, b): seed of one call from a device generator's (seed, offset) without touching the device"""
    x = (a * 0x9E3779B97F4A7C15 + b + 0x632BE59BD9B4E019) & 0xffffffffffffffff
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xffffffffffffffff
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xffffffffffffffff
    return x ^ (x >> 31)


def _draw_seed(generator: Optional[torch.Generator]) -> int:
    """64-bit seed of one sketch.  Host generators (the default one included) are advanced by one draw; a device generator
    is advanced by bumping its Philox offset -- neither reads back from the device."""
    if generator is None or generator.device.type == 'cpu':
        return int(torch.randint(0, 2**62, (), dtype=torch.int64, generator=generator).item())
    offset = generator.get_offset()
    generator.set_offset(offset + 4)
    return _mix64(generator.initial_seed(), offset)


_REPLAY_COUNTERS = {}


def _replay_counter(device: torch.device) -> torch.Tensor:
    """One int64 word per device that the recorded seed kernels advance.  It must exist BEFORE a capture starts (a tensor
    allocated while capturing belongs to the graph's pool and its zero-fill would be replayed too): every eager call of the
    native path makes sure it does, so the customary warm-up run before `torch.cuda.graph(...)` is enough."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    counter = _REPLAY_COUNTERS.get(key)
    if counter is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('fewbit.linear_grp: run the layer once on this device before capturing it into a graph '
                               '(the per-device replay counter of the sketch seeds cannot be created during capture)')
        counter = _REPLAY_COUNTERS[key] = torch.zeros(1, dtype=torch.int64, device=device)
    return counter


_WARNED_CAPTURE_GENERATOR = False


def _warn_device_generator_in_capture() -> None:
    global _WARNED_CAPTURE_GENERATOR
    if not _WARNED_CAPTURE_GENERATOR:
        _WARNED_CAPTURE_GENERATOR = True
        import warnings
        warnings.warn('fewbit.linear_grp: a device generator passed while the stream is being captured into a graph only contributes its '
                      'initial seed -- its offset is not advanced, and replays draw from (that seed, the per-device replay counter); '
                      'eager and captured runs with the same generator therefore see different sketches', RuntimeWarning, stacklevel=4)


def _sketch_seed(generator: Optional[torch.Generator], device: torch.device):
    """Seed of one sketch: an int drawn on the host -- or, while the stream is being captured into a hipGraph, a device word
    that a recorded kernel re-derives from (a host draw made at capture time, the replay counter) on every replay, so that a
    replayed training step meets a fresh S each time instead of the one matrix whose seed was recorded."""
    counter = _replay_counter(device)
    if not torch.cuda.is_current_stream_capturing():
        return _draw_seed(generator)
    from . import cabi
    # (while capturing, a DEVICE generator's offset is not touched: reading or moving it belongs to the graph machinery of
    # torch.cuda; a host generator is used as given.  The counter is one word per device shared by every captured graph: graphs replayed one after the other
    # see consecutive counts (reproducible), graphs replayed CONCURRENTLY on several streams still get distinct counts -- the
    # bump is an atomic add -- but which graph gets which is then up to the hardware.)
    if generator is not None and generator.device.type != 'cpu':
        # the user's generator still determines the stream: the base of the recorded seed kernel is derived from its initial seed
        # (a host-side read; its offset is neither read nor moved) and the per-device replay counter, so two captures with
        # generators of different seeds draw different matrices, and the host's global RNG state is left alone
        _warn_device_generator_in_capture()
        return cabi.next_sketch_seed(counter, _mix64(generator.initial_seed(), 0x6361707475726564))
    return cabi.next_sketch_seed(counter, _draw_seed(generator))


def _kernel_rows(mat: torch.Tensor) -> bool:
    """whether the rows of ``mat`` are unit-stride rows at least ``features`` apart: what the kernels take as it is"""
    return mat.stride(1) == 1 and mat.stride(0) >= mat.shape[1]


def _unit_stride(mat: torch.Tensor) -> torch.Tensor:
    """``mat``, or a contiguous copy when the kernels do not take its rows (e.g. the expanded gradient of a sum: strides (0, 0))"""
    return mat if _kernel_rows(mat) else mat.contiguous()


def _native_sketch(kind: str, mat: torch.Tensor, p: int, seed, scale: float) -> torch.Tensor:
    """the dense leg of _native_project (a seam of its own: tests count the dense products of a step through it)"""
    from . import cabi
    return cabi.sketch(kind, _unit_stride(mat), p, seed, scale)


def _native_project(kind: str, mat: torch.Tensor, p: int, seed, scale: float, rows: int = 0, out_dtype: Optional[torch.dtype] = None,
                    signed: bool = False) -> torch.Tensor:
    """One estimator product on this package's kernels, the only place that picks the binding.  'gaussian' / 'rademacher': ``scale * S(seed) @ mat``.
    'dct' / 'dft': ``scale * transform(mat, dim=0, norm='ortho')[rows(seed)]`` on the kernel pair: M is read once, one fp32 intermediate goes
    out and back, only the p sampled rows are written (the torch formulation materialises the whole transform in fp32 first).  'dct': a
    ``(p, features)`` tensor of the dtype of ``mat``; 'dft': a ``(2, p, features)`` tensor of ``out_dtype`` (default: the dtype of ``mat``),
    ``[0]`` the real part, ``[1]`` the imaginary part.  ``rows`` other than 0 and the rows of ``mat``: the transform of that length of ``mat``
    followed by zero rows (the zero-extended pair; the sampled rows are those of ``seed`` in ``[0, rows)``).  ``signed``: 'dct' / 'dft' of
    ``mat`` with the rows of ``cabi_x.sampled_signs(seed, mat.shape[0])`` negated (the signed pair, at either length)"""
    if kind in ('gaussian', 'rademacher'):
        return _native_sketch(kind, mat, p, seed, scale)
    mat = _unit_stride(mat)
    if signed:
        from . import cabi_x
        if kind == 'dct':
            return cabi_x.sampled_dct_signed(mat, rows or mat.shape[0], p, seed, scale)
        return cabi_x.sampled_dft_signed(mat, rows or mat.shape[0], p, seed, scale, out_dtype)
    if rows and rows != mat.shape[0]:
        from . import cabi_x
        if kind == 'dct':
            return cabi_x.sampled_dct_zext_seeded(mat, rows, p, seed, scale)
        return cabi_x.sampled_dft_zext_seeded(mat, rows, p, seed, scale, out_dtype)
    if kind == 'dct':
        from . import cabi
        return cabi.sampled_dct_seeded(mat, p, seed, scale)
    from . import cabi_x
    return cabi_x.sampled_dft_seeded(mat, p, seed, scale, out_dtype)


_INJECTED: Optional[torch.Tensor] = None


@contextlib.contextmanager
def inject_sketch(S: torch.Tensor):
    """Checker hook: inside the block every dense sketch (forward AND backward of ``linear_grp`` with ``'gaussian'`` /
    ``'rademacher'``) is the given ``p x rows`` matrix instead of a fresh draw.  The fixture tests inject the matrix the
    reference drew (tests/golden/linear_draw_ref.npz) and compare the weight gradient with the reference's own."""
    global _INJECTED
    prev, _INJECTED = _INJECTED, S
    try:
        yield
    finally:
        _INJECTED = prev


def _dense_sketch(kind: str, p: int, rows: int, like: torch.Tensor, gen: torch.Generator,
                  draw_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    if _INJECTED is not None:
        if tuple(_INJECTED.shape) != (p, rows):
            raise ValueError(f'injected sketch is {tuple(_INJECTED.shape)}, this call needs {(p, rows)}')
        return _INJECTED.to(like.device, like.dtype)
    if kind == 'gaussian':
        # drawn in ONE dtype (`draw_dtype`, recorded by the forward) and then cast to the operand: randn's stream depends
        # on the dtype, so a backward whose grad_output has another dtype than the forward's input (autocast) would
        # otherwise replay a different S and return pure noise
        return torch.randn((p, rows), generator=gen, device=gen.device, dtype=draw_dtype or like.dtype).to(like.device, like.dtype)
    signs = torch.randint(0, 2, (p, rows), generator=gen, device=gen.device, dtype=torch.int8).to(like.device)
    return (signs.to(like.dtype) * 2) - 1                                       # Rademacher: +-1


def _flipped_rows(mat: torch.Tensor, gen: torch.Generator) -> torch.Tensor:
    """``D mat`` for a ``D = diag(+-1)`` drawn from ``gen`` (one draw of ``rows`` bits; negation is exact in every dtype)"""
    flip = torch.randint(0, 2, (mat.shape[0], ), generator=gen, device=gen.device, dtype=torch.int8).to(mat.device).bool()
    return torch.where(flip.unsqueeze(1), -mat, mat)


def _sampled_rows(p: int, rows: int, like: torch.Tensor, gen: torch.Generator) -> torch.Tensor:
    return torch.randint(0, rows, (p, ), generator=gen, device=gen.device).to(like.device)


_TRANSFORM_ROWS = {}


def _transform_rows(kind: str, rows: int) -> bool:
    """Whether the library that owns the sampled transform ``kind`` has a kernel for ``rows`` rows, as it says itself: its workspace query
    at (rows, 1, 1) is non-zero ('dct': libfewbit_hip.so, 'dft': libfewbit_hipx.so -- a 'dct' question never loads the companion library);
    asked once per kind and row count."""
    ok = _TRANSFORM_ROWS.get((kind, rows))
    if ok is None:
        if kind == 'dct':
            from . import cabi
            ok = cabi.sampled_dct_workspace_bytes(rows, 1, 1, torch.float32) != 0
        else:
            from . import cabi_x
            ok = cabi_x.sampled_dft_workspace_bytes(rows, 1, 1, torch.float32) != 0
        _TRANSFORM_ROWS[(kind, rows)] = ok
    return ok


def _zext_span_ok(rows: int, ld: int, itemsize: int) -> bool:
    """Whether ``rows x ld`` elements lie in the span the zero-extended pass A addresses (its buffer descriptor is 32 bits wide:
    fewbit_fft4.h::zext_span_ok, the same bound)"""
    return rows * ld * itemsize <= 0xfffffff0


def _native_transform_rows(kind: str, mat: torch.Tensor) -> int:
    """The row count at which the gfx950 sampled-transform kernel pairs (fewbit_amd/csrc/fewbit_dct.hip, fewbit_dft.hip) run ``mat``; 0: they
    do not.  They take 2-D fp32 / fp16 / bf16 GPU tensors of the row counts their library has a kernel for (_transform_rows; e.g. RoBERTa's
    128 x 128 tokens = 16384, 32 sequences of 384 tokens = 12288 = 3 x 2^12, 28 sequences of 128 tokens = 3584 = 7 x 2^9): the rows of
    ``mat``.  With ``use_row_extension()`` on, any other row count up to 262144 runs zero-extended at the next supported one
    (``cabi_x.sampled_rows_ceil``) -- unless the matrix spans 4 GiB or more, which the zero-extended pass A does not address.  Everything
    else keeps the torch.fft formulation."""
    if not (_NATIVE_SKETCH and kind in ('dct', 'dft') and mat.device.type == 'cuda' and mat.dim() == 2
            and mat.dtype in (torch.float32, torch.float16, torch.bfloat16) and mat.shape[1] > 0):
        return 0
    rows = mat.shape[0]
    if _transform_rows(kind, rows):
        return rows
    if not _EXTEND_ROWS or rows < 1:
        return 0
    ld = mat.stride(0) if _kernel_rows(mat) else mat.shape[1]      # (what _unit_stride hands the kernels)
    if not _zext_span_ok(rows, ld, mat.element_size()):
        return 0
    from . import cabi_x
    return cabi_x.sampled_rows_ceil(rows)


_TRANSFORM_PATHS = {
    'dct': 'gfx950 kernel pair fewbit_hip_sampled_dct (four-step fp32 FFT in LDS, only the sampled rows are written; in the layer: rows of a seed)',
    'dft': ('gfx950 kernel pair fewbit_hipx_sampled_dft (four-step fp32 FFT in LDS, only the sampled rows are written, real and imaginary '
            'planes; in the layer: rows of a seed)'),
}


def sampled_transform_path(kind: str, mat: torch.Tensor) -> str:
    """Which code computes the sampled transform ``kind`` ('dct' / 'dft') of ``mat`` (what bench.py prints beside its time)."""
    rows = _native_transform_rows(kind, mat)
    if rows and _SIGN_FLIPS:
        planes = '' if kind == 'dct' else ', real and imaginary planes'
        length = '' if rows == mat.shape[0] else f', zero-extended to {rows} rows'
        return (f'gfx950 kernel pair fewbit_hipx_sampled_{kind}_signed{length} (rows negated by the signs of the seed as pass A loads them, '
                f'four-step fp32 FFT in LDS, only the sampled rows are written{planes}; in the layer: rows and signs of one seed)')
    if rows == mat.shape[0] and rows:
        return _TRANSFORM_PATHS[kind]
    if rows:
        planes = '' if kind == 'dct' else ', real and imaginary planes'
        return (f'gfx950 kernel pair fewbit_hipx_sampled_{kind}_zext, zero-extended to {rows} rows (four-step fp32 FFT in LDS, the missing rows are '
                f'never loaded, only the sampled rows are written{planes}; in the layer: rows of a seed; an unbiased estimator, not the '
                "reference's transform at the true length)")
    signs = 'rows negated by random signs of the generator, then ' if _SIGN_FLIPS else ''
    return f'torch.fft (rocFFT on the GPU): {signs}full transform along dim 0 in fp32, then the gather of the sampled rows'


def sampled_transform(kind: str, mat: torch.Tensor, p: int, gen: torch.Generator, seed: int = 1234, scale: float = 1.0) -> torch.Tensor:
    """One estimator product of the layer, ``scale * transform(mat)[p sampled rows]``, on the path ``linear_grp`` takes for this
    ``kind`` and ``mat`` (what bench.py and tools/ time): the kernel pair with rows of ``seed``, or torch.fft + randint from ``gen``.
    'dft' returns a complex64 ``(p, features)`` tensor on either path (on the kernel pair: built from its fp32 planes).  With
    ``use_sign_flips()`` on, the rows are negated by the signs of ``seed`` (kernel pair) or of ``gen`` (torch.fft) first."""
    rows = _native_transform_rows(kind, mat)                  # (other than the rows of mat: the zero-extended pair, rows of seed in [0, rows))
    if not rows:
        return _sketch(kind, mat, p, gen, scale=scale, signed=_SIGN_FLIPS)
    if kind == 'dct':
        return _native_project(kind, mat, p, seed, scale, rows, signed=_SIGN_FLIPS)
    planes = _native_project(kind, mat, p, seed, scale, rows, torch.float32, signed=_SIGN_FLIPS)
    return torch.complex(planes[0], planes[1])


def _sketch(kind: str, mat: torch.Tensor, p: int, gen: torch.Generator, sketch_dtype=None, draw_dtype=None, scale: float = 1.0,
            signed: bool = False) -> torch.Tensor:
    """``scale * S @ mat`` (``E[S^T S] = p * I`` for the dense sketches, ``(p / rows) * I`` for the sampled transforms).  ``signed``: the
    sampled transforms of ``D mat``, ``D = diag(+-1)`` drawn from ``gen`` BEFORE the rows (a replay draws in the same order)."""
    rows = mat.shape[0]
    if kind in ('gaussian', 'rademacher'):
        if sketch_dtype is not None and sketch_dtype != mat.dtype:
            low = mat.to(sketch_dtype)
            out = (_dense_sketch(kind, p, rows, low, gen, draw_dtype) @ low).to(mat.dtype)
        else:
            out = _dense_sketch(kind, p, rows, mat, gen, draw_dtype) @ mat
        return out if scale == 1.0 else out * scale
    if signed:
        mat = _flipped_rows(mat, gen)
    idx = _sampled_rows(p, rows, mat, gen)
    if kind == 'dct':
        out = dct(mat, dim=0, norm='ortho')[idx]
        return out if scale == 1.0 else out * scale
    work = mat if mat.dtype in (torch.float32, torch.float64) else mat.float()
    out = torch.fft.fft(work, dim=0, norm='ortho')[idx]                         # complex
    return out if scale == 1.0 else out * scale


def _autocast_seen(device_type: str):
    """the autocast state of the calling thread for ``device_type``, as a forward records it for its backward"""
    enabled = torch.is_autocast_enabled(device_type)
    return device_type, enabled, torch.get_autocast_dtype(device_type) if enabled else None


def _autocast_as(seen):
    """Context in which a backward runs under the autocast state its forward saw (what ``torch.amp.custom_bwd`` does; one Function serves
    host and GPU tensors here, so the device type is the input's, recorded by the forward).  A plain ``autograd.Function``'s backward runs
    under the state of the thread that calls ``backward()``: after the ``autocast`` block is left -- the ordinary AMP pattern -- a bf16
    ``grad_output`` would meet the fp32 weight uncast.  No autocast in forward: disabled in backward, whatever the caller's state."""
    device_type, enabled, dtype = seen
    if torch.is_autocast_enabled(device_type) == enabled and (not enabled or torch.get_autocast_dtype(device_type) == dtype):
        return contextlib.nullcontext()
    return torch.autocast(device_type, dtype=dtype, enabled=enabled)


def _dense_rows(grad_output: torch.Tensor) -> torch.Tensor:
    """``grad_output`` as backward works on it: itself when contiguous (the usual case, no copy), else a contiguous copy -- the expanded
    gradient of a ``sum()``, a transposed tensor.  The order in which ``sum(dim=0)`` and the library GEMMs add depends on the strides of
    their operands, so without it one gradient in two layouts gave two results that differ in their last bits."""
    return grad_output if grad_output.is_contiguous() else grad_output.contiguous()


def _plain_linear(input: torch.Tensor, weight: torch.Tensor) -> bool:
    """Whether a call is ``F.linear`` and nothing else: no weight gradient can follow (grad mode is off -- ``no_grad``, ``inference_mode``,
    the first pass of a re-entrant checkpoint -- or the weight is frozen; ``ctx.needs_input_grad`` does not show grad mode), or there are no
    rows to sketch (the weight gradient of ``F.linear`` is then exactly zero).  No seed is drawn, nothing is launched, nothing is saved."""
    return not torch.is_grad_enabled() or not weight.requires_grad or input.numel() == 0


class _LinearGRP(torch.autograd.Function):

    @staticmethod
    def forward(ctx, input, weight, bias, p: int, kind: str, generator, sketch_dtype=None):
        flat = input.reshape(-1, input.shape[-1])
        rows = flat.shape[0]
        ctx.p, ctx.kind = p, kind
        ctx.autocast = _autocast_seen(input.device.type)
        ctx.has_bias = bias is not None
        # the route, decided here once: None -- the PyTorch formulation; 0 -- the dense kernel; N' -- the sampled-transform pair at N' rows: the
        # rows of flat, or with use_row_extension() the next supported count (flat zero-extended; the rows of the seed are drawn from [0, N'),
        # the scale is N' / p, and backward runs on the same N' and seed)
        dense = _native_sketch_applies(kind, flat, sketch_dtype)
        ctx.route = 0 if dense else _native_transform_rows(kind, flat) or None
        ctx.signed = _SIGN_FLIPS and kind in ('dct', 'dft')                # (recorded: backward flips iff forward did, whatever the switch says then)
        if ctx.route is not None:
            # S -- or the sampled rows -- lives nowhere: a function of the seed that the kernel evaluates itself; the projection and the
            # seed are all that is kept (no randint launch, no RNG state to save and replay; while a graph is being captured the seed is
            # a device word)
            ctx.native_seed = _sketch_seed(generator, flat.device)
            # sketch_dtype (16-bit) for a wider input: a dense projection is computed from, and KEPT in, that dtype -- half the saved bytes
            # of an fp32 layer, and the small GEMM of backward runs on the 16-bit matrix pipe as well
            ctx.low = sketch_dtype if dense and sketch_dtype is not None and sketch_dtype != flat.dtype else None
            x = flat.detach() if ctx.low is None else flat.detach().to(ctx.low)
            # (the sketch before or after the layer's own GEMM: no difference, profiles/r05_roberta_ab_order.txt)
            kept = _native_project(kind, x, p, ctx.native_seed, (ctx.route or 1) / p, ctx.route, signed=ctx.signed)
            # ('dft': the real and imaginary planes in the layer's dtype, two views of one buffer)
            ctx.save_for_backward(*((kept[0], kept[1]) if kind == 'dft' else (kept, )), weight)
            return F.linear(input, weight, bias)
        token, gen = _capture_rng(generator, input.device)
        scale = 1.0 / p if kind in ('gaussian', 'rademacher') else rows / p
        draw_dtype = sketch_dtype or flat.dtype
        sketch = _sketch(kind, flat.detach(), p, gen, sketch_dtype, draw_dtype, scale, ctx.signed)
        ctx.save_for_backward(sketch, weight)
        ctx.token, ctx.sketch_dtype, ctx.draw_dtype = token, sketch_dtype, draw_dtype
        return F.linear(input, weight, bias)

    @staticmethod
    def backward(ctx, grad_output):
        with _autocast_as(ctx.autocast):
            return _LinearGRP._backward(ctx, _dense_rows(grad_output))

    @staticmethod
    def _backward(ctx, grad_output):
        saved = ctx.saved_tensors                       # (sketch, weight); 'dft' on the kernel pair: (real plane, imaginary plane, weight)
        sketch, weight = saved[0], saved[-1]
        grad_input = grad_weight = grad_bias = None
        if ctx.needs_input_grad[0]:
            grad_input = grad_output @ weight
        flat = grad_output.reshape(-1, grad_output.shape[-1])
        if ctx.needs_input_grad[1] and ctx.route is not None:
            # the same S again, from the same seed (a grad_output of another dtype than the forward's input -- autocast --
            # still meets the same matrix: S does not depend on the operand dtype beyond its final rounding)
            g2 = flat if flat.dtype in (torch.float32, torch.float16, torch.bfloat16) else flat.float()
            if ctx.low is not None:
                g2 = g2.to(ctx.low)
            proj = _native_project(ctx.kind, g2, ctx.p, ctx.native_seed, 1.0, ctx.route, signed=ctx.signed).to(sketch.dtype)
            if len(saved) == 3:                         # Re((F G)^H (F X)) = Gr^T Xr + Gi^T Xi: two accumulating GEMMs in the dtype of the planes
                grad_weight = torch.addmm(proj[0].T @ saved[0], proj[1].T, saved[1]).to(weight.dtype)
            else:
                grad_weight = (proj.T @ sketch).to(weight.dtype)
        elif ctx.needs_input_grad[1]:
            proj = _sketch(ctx.kind, flat, ctx.p, _replay_rng(ctx.token), ctx.sketch_dtype, ctx.draw_dtype, signed=ctx.signed)
            if proj.is_complex():                                               # Re((F G)^H (F X))
                grad_weight = (proj.real.T @ sketch.real + proj.imag.T @ sketch.imag).to(weight.dtype)
            else:
                grad_weight = (proj.T @ sketch).to(weight.dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            grad_bias = flat.sum(dim=0)
        return grad_input, grad_weight, grad_bias, None, None, None, None


def linear_grp(input: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
               proj_dim_ratio: Optional[float] = None, proj_dim: Optional[int] = None,
               proj_dim_max: Optional[int] = None, proj_dim_min: Optional[int] = None, matmul: str = 'gaussian',
               generator: Optional[torch.Generator] = None, sketch_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``F.linear(input, weight, bias)`` whose weight gradient is estimated through a random projection of the rows
    (argument order of the reference's ``linear_grp``, fewbit/functional/linear.py:85-90)."""
    if proj_dim_ratio is None and proj_dim is None:
        raise ValueError('Either proj_dim or proj_dim_ratio should be specified.')
    if proj_dim_min is not None and proj_dim_min <= 0:
        raise ValueError('Param proj_dim_min should be strictly positive.')
    if proj_dim_min and proj_dim_max and proj_dim_max < proj_dim_min:
        raise ValueError('Param proj_dim_min should be not greater than param proj_dim_max.')
    if matmul not in MATMUL_TYPES:
        raise ValueError(f'Unexpected matmul type: {matmul}.')
    if _plain_linear(input, weight):
        return F.linear(input, weight, bias)
    rows = input.numel() // input.shape[-1]
    p = projection_dim(rows, proj_dim_ratio, proj_dim, proj_dim_max, proj_dim_min)
    return _LinearGRP.apply(input, weight, bias, p, matmul, generator, sketch_dtype)


linear_randomized = linear_grp


_CRS_SHAPES = {}


def _native_crs_applies(flat: torch.Tensor, weight: torch.Tensor, nopairs: int) -> bool:
    """The gfx950 column-sampling kernels (fewbit_amd/csrc/fewbit_crs.hip) take fp32 / fp16 / bf16 GPU tensors of the shapes the companion
    library says it has a kernel for (its workspace query is non-zero; asked once per shape); everything else keeps the PyTorch formulation."""
    if not (_NATIVE_SKETCH and flat.device.type == 'cuda' and flat.dtype in (torch.float32, torch.float16, torch.bfloat16)
            and weight.dtype == flat.dtype and weight.device == flat.device):
        return False
    key = (flat.dtype, flat.shape[0], flat.shape[1], nopairs)
    ok = _CRS_SHAPES.get(key)
    if ok is None:
        from . import cabi_x
        ok = _CRS_SHAPES[key] = cabi_x.crs_workspace_bytes(flat.shape[0], flat.shape[1], nopairs, flat.dtype) != 0
    return ok


class _LinearCRS(torch.autograd.Function):
    """Column sampling of the weight gradient: ``nopairs`` draws (with replacement) from the ``in_features`` columns;
    only the drawn columns of the input are kept, each scaled by ``count / (nopairs / in_features)`` so that the
    estimate is unbiased (behaviour of fewbit/functional/linear.py:28-62).

    On the GPU (fp32 / fp16 / bf16, ``use_native_sketch()`` on) the drawn columns are, like the sampled rows of 'dct' / 'dft', a function of
    the call's 64-bit seed (``_sketch_seed``: the host default generator, so ``torch.manual_seed`` reproduces a run) that the kernels of
    ``fewbit_amd/csrc/fewbit_crs.hip`` evaluate themselves (``cabi_x.crs_columns`` is the same function on the host): forward is ONE call that
    gathers and scales the drawn columns (the scale is applied in fp32, the result rounded once to the layer's dtype), backward is the
    library GEMM ``G^T kept`` and ONE call that writes all of ``dL/dW``.  Kept for backward: the ``rows x m`` projection (``m`` distinct
    columns, known from the host evaluation of the seed) and one integer -- no column list, no randint / bincount / nonzero, no read-back
    and no stream synchronisation.  While the stream is being captured into a hipGraph the seed is a device word the host cannot evaluate:
    the projection then has ``cap = min(nopairs, in_features)`` columns, the ``cap - m`` unused ones exactly zero, and every replay draws
    fresh columns.  Host tensors, float64, ``use_native_sketch(False)`` and shapes the library has no kernel for take the PyTorch
    formulation below, whose ``nonzero`` reads the number of hit columns back from the device (and cannot be captured)."""

    @staticmethod
    def forward(ctx, input, weight, bias, nopairs: int):
        in_features = weight.shape[1]
        ctx.has_bias = bias is not None
        ctx.native_seed = None
        ctx.autocast = _autocast_seen(input.device.type)
        flat = input.detach().reshape(-1, in_features)
        if _native_crs_applies(flat, weight, nopairs):
            from . import cabi_x
            ctx.native_seed, ctx.nopairs = _sketch_seed(None, flat.device), nopairs
            ctx.save_for_backward(cabi_x.crs_gather(_unit_stride(flat), ctx.native_seed, nopairs), weight)
            return F.linear(input, weight, bias)
        draws = torch.randint(0, in_features, (nopairs, ), device=input.device)
        counts = torch.bincount(draws, minlength=in_features)
        scale = counts.to(input.dtype) * (in_features / nopairs)
        # a dense (rows x in_features) product with a mostly-zero scale would save nothing: keep the hit columns only.
        # nonzero() has a data-dependent size and therefore reads back from the device -- the price of drawing the columns on the device with
        # torch's generator; the kernels above avoid it by making the columns a function of a seed that the host can evaluate as well.
        cols = torch.nonzero(counts, as_tuple=True)[0]
        ctx.save_for_backward(flat[:, cols] * scale[cols], weight, cols)
        return F.linear(input, weight, bias)

    @staticmethod
    def backward(ctx, grad_output):
        with _autocast_as(ctx.autocast):
            return _LinearCRS._backward(ctx, _dense_rows(grad_output))

    @staticmethod
    def _backward(ctx, grad_output):
        saved = ctx.saved_tensors                       # read once: a non-re-entrant checkpoint unpacks a saved tensor one time only
        kept, weight = saved[:2]
        grad_input = grad_weight = grad_bias = None
        if ctx.needs_input_grad[0]:
            grad_input = grad_output @ weight
        flat = grad_output.reshape(-1, grad_output.shape[-1])
        if ctx.needs_input_grad[1] and ctx.native_seed is not None:
            from . import cabi_x
            t = (flat.T @ kept).to(weight.dtype)
            grad_weight = cabi_x.crs_scatter(t.contiguous(), ctx.native_seed, weight.shape[1], ctx.nopairs)
        elif ctx.needs_input_grad[1]:
            cols = saved[2]
            grad_weight = torch.zeros_like(weight)
            grad_weight[:, cols] = (flat.T @ kept).to(weight.dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            grad_bias = flat.sum(dim=0)
        return grad_input, grad_weight, grad_bias, None


def linear_crs(input: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], nopairs: int) -> torch.Tensor:
    """``F.linear`` with a column-sampled weight gradient (reference: ``linear_crs``, fewbit/functional/linear.py:65)."""
    if nopairs < 1:
        raise ValueError('Number of sampled pairs should be strictly positive.')
    if _plain_linear(input, weight):
        return F.linear(input, weight, bias)
    return _LinearCRS.apply(input, weight, bias, int(nopairs))


# ---- every element of the input in 2, 4 or 8 bits --------------------------------------------------------------------------------------

# the code widths: the binding's constant (the import loads no library).  What the node keeps, and how it is decoded and multiplied: ``kept``
from . import kept  # noqa: E402
from .cabi import DTYPES as _DTYPES  # noqa: E402
from .cabi_x import QUANT_BITS  # noqa: E402
from .kept import decode_in_two_terms as _decode_in_two_terms, two_term_product as _two_term_product  # noqa: E402,F401  (their names here: tests use them)


def _kernels_take(t: torch.Tensor) -> bool:
    """Whether ``t`` is a tensor the quantizing kernels take: fp32 / fp16 / bf16, on the GPU, 1 .. 2^36 elements, while ``use_native_sketch()`` is on"""
    return _NATIVE_SKETCH and t.device.type == 'cuda' and t.dtype in _DTYPES and 0 < t.numel() <= 2**36


def _native_quant_applies(flat: torch.Tensor) -> bool:
    """The gfx950 kernels (fewbit_amd/csrc/fewbit_quant.hip) take fp32 / fp16 / bf16 GPU tensors of up to 2^36 elements"""
    return _kernels_take(flat)


class _LinearQuantized(torch.autograd.Function):
    """``F.linear`` that keeps its input in ``bits`` bits per element for the weight gradient (module docstring).  Kept for backward on the
    kernels: ONE uint8 buffer (``cabi_x.quant_pack``), the weight, the seed (an int; a device word while the stream is being captured) and
    the shape; in the PyTorch formulation the codes (one per byte) and the two parameters of every group."""

    @staticmethod
    def forward(ctx, input, weight, bias, bits: int, generator):
        flat = input.detach().reshape(-1, input.shape[-1])
        ctx.bits, ctx.flat_shape = bits, tuple(flat.shape)
        ctx.has_bias = bias is not None
        ctx.autocast = _autocast_seen(input.device.type)
        ctx.native_seed = _sketch_seed(generator, flat.device) if _native_quant_applies(flat) else None
        ctx.save_for_backward(*kept.keep(flat, bits, ctx.native_seed, generator), weight)
        return F.linear(input, weight, bias)

    @staticmethod
    def backward(ctx, grad_output):
        with _autocast_as(ctx.autocast):
            return _LinearQuantized._backward(ctx, _dense_rows(grad_output))

    @staticmethod
    def _backward(ctx, grad_output):
        *x_kept, weight = ctx.saved_tensors             # read once: a non-re-entrant checkpoint unpacks a saved tensor one time only
        grad_input = grad_weight = grad_bias = None
        if ctx.needs_input_grad[0]:
            grad_input = grad_output @ weight
        flat = grad_output.reshape(-1, grad_output.shape[-1])
        if ctx.needs_input_grad[1]:
            # X^ in the gradient's dtype (under autocast not the input's): a transient tensor, one GEMM (the kernels decode into fp32 / fp16 / bf16)
            g2 = flat if ctx.native_seed is None or flat.dtype in _DTYPES else flat.float()
            grad_weight = kept.products((g2, ), x_kept, ctx.flat_shape, ctx.bits)[0].to(weight.dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            grad_bias = flat.sum(dim=0)
        return grad_input, grad_weight, grad_bias, None, None


def linear_quantized(input: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, bits: int = 4,
                     generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """``F.linear(input, weight, bias)`` that keeps its input in ``bits`` = 2, 4 or 8 bits per element, rounded without bias, for the weight
    gradient: ``grad_input`` and ``grad_bias`` are exact, ``grad_weight = G^T X^`` (module docstring).  ``generator``: the source of the
    rounding's randomness; without it the host default generator seeds every call."""
    kept.check_bits(bits)
    if _plain_linear(input, weight):
        return F.linear(input, weight, bias)
    return _LinearQuantized.apply(input, weight, bias, int(bits), generator)


# ---- modules ---------------------------------------------------------------------------------------------------------

class LinearCRS(torch.nn.Linear):
    """:class:`torch.nn.Linear` whose weight gradient is estimated from ``proj_dim`` sampled input columns
    (default ``out_features // 2``, as in fewbit/modules/linear.py:22-36; the reference's constructor forwards
    ``proj_dim`` into the ``bias`` slot of ``nn.Linear`` and its ``extra_repr`` reads an undefined attribute --
    both fixed here)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True, device=None, dtype=None,
                 proj_dim: Optional[int] = None) -> None:
        super().__init__(in_features, out_features, bias, device, dtype)
        self.proj_dim: int = proj_dim or max(out_features // 2, 1)

    @property
    def nopairs(self) -> int:
        return self.proj_dim

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        return linear_crs(input, self.weight, self.bias, self.proj_dim)

    def extra_repr(self) -> str:
        return f'{super().extra_repr()}, nopairs={self.nopairs}'


class LinearGRP(torch.nn.Linear):
    r"""Drop-in :class:`torch.nn.Linear` (:math:`y = xA^T + b`) that stores a random projection of its input along
    the batch dimension instead of the input itself and estimates the weight gradient from it.

    Parameters (after those of ``nn.Linear``; either ``proj_dim_ratio`` or ``proj_dim`` is required)
    ----------
    proj_dim_ratio : float, optional
        ``proj_dim`` as a fraction of the number of input rows.
    proj_dim : int, optional
        Exact number of rows of the projection.
    proj_dim_min, proj_dim_max : int, optional
        Bounds on the number of rows.
    matmul : {'dct', 'dft', 'gaussian', 'rademacher'}, default='gaussian'
        Kind of random projection.
    generator : torch.Generator, optional
        Source of randomness; without it the host default generator seeds every call.  Inside ``torch.utils.checkpoint`` it must be a
        DEFAULT generator (``None``, ``torch.default_generator`` or ``torch.cuda.default_generators[i]``): checkpoint saves and restores
        only those, so with any other generator the recomputation draws a second seed -- in non-reentrant mode the layers behind this one
        then receive activations recomputed under another sketch than the one this layer's backward uses, in reentrant mode every
        gradient belongs to another sketch than the output.  With a default generator both modes give the plain run's bits.
    sketch_dtype : torch.dtype, optional
        dtype of the dense sketch products (extension; e.g. ``torch.bfloat16`` for an fp32 layer on the GPU).

    Examples:

        >>> m = fewbit.RandomizedLinear(20, 30, proj_dim_ratio=0.5)
        >>> m(torch.randn(128, 20)).size()
        torch.Size([128, 30])
    """

    def __init__(self, in_features: int, out_features: int, bias: bool = True, device=None, dtype=None,
                 proj_dim_ratio: Optional[float] = None, proj_dim: Optional[int] = None,
                 proj_dim_min: Optional[int] = None, proj_dim_max: Optional[int] = None, matmul: str = 'gaussian',
                 generator: Optional[torch.Generator] = None, sketch_dtype: Optional[torch.dtype] = None) -> None:
        super().__init__(in_features, out_features, bias, device, dtype)
        self.generator = generator
        self.sketch_dtype = sketch_dtype
        self.matmul = matmul
        self.proj_dim_ratio = proj_dim_ratio
        self.proj_dim = proj_dim
        self.proj_dim_max = proj_dim_max
        self.proj_dim_min = proj_dim_min

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        return linear_grp(input, self.weight, self.bias, self.proj_dim_ratio, self.proj_dim, self.proj_dim_max,
                          self.proj_dim_min, self.matmul, self.generator, self.sketch_dtype)

    def extra_repr(self) -> str:
        return ', '.join([super().extra_repr(), f'matmul={self.matmul}', f'proj_dim={self.proj_dim}',
                          f'proj_dim_ratio={self.proj_dim_ratio}', f'proj_dim_max={self.proj_dim_max}',
                          f'proj_dim_min={self.proj_dim_min}'])


RandomizedLinear = LinearGRP


class QuantizedLinear(torch.nn.Linear):
    r"""Drop-in :class:`torch.nn.Linear` that keeps its input in ``bits`` bits per element instead of the input itself and forms the weight
    gradient from the decoded values; the output, the input gradient and the bias gradient are those of ``nn.Linear``.

    Parameters (after those of ``nn.Linear``)
    ----------
    bits : {2, 4, 8}, default=4
        Bits per kept element.  Groups of 64 elements share a minimum and a step (8 more bytes per group): a bf16 input is kept in 0.1875,
        0.3125 or 0.5625 of its bytes.  The rounding is stochastic and unbiased; the error of an element is below its group's step.  With bf16
        gradients, 8 bits cost about twice the backward time of 2 or 4 (the decode is then multiplied as two bf16 terms to stay unbiased).
    generator : torch.Generator, optional
        Source of the rounding's randomness; without it the host default generator seeds every call.  Inside ``torch.utils.checkpoint`` it
        must be a default generator, as for :class:`LinearGRP`.

    Examples:

        >>> m = fewbit.QuantizedLinear(20, 30, bits=4)
        >>> m(torch.randn(128, 20)).size()
        torch.Size([128, 30])
        >>> model = fewbit.map_module(model, lambda m, path: fewbit.QuantizedLinear.from_linear(m, bits=4) if type(m) is torch.nn.Linear else m)
    """

    def __init__(self, in_features: int, out_features: int, bias: bool = True, device=None, dtype=None, bits: int = 4,
                 generator: Optional[torch.Generator] = None) -> None:
        kept.check_bits(bits)
        super().__init__(in_features, out_features, bias, device, dtype)
        self.bits = bits
        self.generator = generator

    @classmethod
    def from_linear(cls, module: torch.nn.Linear, bits: int = 4, generator: Optional[torch.Generator] = None) -> 'QuantizedLinear':
        """A ``QuantizedLinear`` that SHARES the parameters of ``module`` (what ``map_module`` needs to swap the linears of a built model)"""
        new = cls(module.in_features, module.out_features, module.bias is not None, device='meta', bits=bits, generator=generator)
        new.weight, new.bias = module.weight, module.bias
        return new.train(module.training)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        return linear_quantized(input, self.weight, self.bias, self.bits, self.generator)

    def extra_repr(self) -> str:
        return f'{super().extra_repr()}, bits={self.bits}'
