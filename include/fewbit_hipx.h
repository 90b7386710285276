/*
 * fewbit_hipx.h -- C-ABI of libfewbit_hipx.so, the companion library of libfewbit_hip.so (include/fewbit_hip.h).
 *
 * libfewbit_hip.so is frozen at ABI 5: its exported symbol list does not grow.  Entry points added after that live here, in a
 * library of their own with its own version.  The conventions are fewbit_hip.h's: every pointer is a DEVICE pointer unless
 * stated otherwise; `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work on `stream` and
 * never synchronise; the return value is FEWBIT_OK or a negative fewbit_status, and fewbit_hipx_last_error() gives the message of
 * the last failure on the calling thread.  Kernels launch on the calling thread's current device.  The dtype and status enums
 * are fewbit_hip.h's.  The library does not depend on libfewbit_hip.so; what both evaluate (the rows of a seed, the device seed
 * words of fewbit_hip_sketch_next_seed) is one definition, fewbit_amd/csrc/fewbit_fft4.h and fewbit_philox.h.
 */
#ifndef FEWBIT_HIPX_H_
#define FEWBIT_HIPX_H_

#include <stddef.h>
#include <stdint.h>

#include "fewbit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version history.  Bindings check it and refuse an older library by name.
 *   1: fewbit_hipx_sampled_dft, _seeded, _workspace (the reference's 'dft' estimator).
 * What is declared below is what a binding needs (tests/test_dft_host.py pins the exported symbol list).
 * Additions that leave every version-1 entry point as it was do not move the version; they move the REVISION:
 *   revision 1: the version-1 library as first released (it has no fewbit_hipx_revision symbol).
 *   revision 2: fewbit_hipx_revision; the column sampling of LinearCRS: fewbit_hipx_crs_columns, _crs_workspace, _crs_gather, _crs_scatter.
 * The zero-extended sampled transforms (fewbit_hipx_sampled_rows_ceil, _sampled_dct_zext, _sampled_dft_zext and their _seeded forms) were
 * added inside revision 2: a binding recognises them by the presence of the symbols and refuses by name a library that lacks them.
 * So were the moments of the variance estimator (fewbit_hipx_moments_workspace, _row_moments, _sum_squares): inside revision 2, recognised
 * by the presence of the symbols.
 * So was the dropout whose mask is a function of a seed (fewbit_hipx_dropout_threshold, _dropout_keep, _dropout): inside revision 2,
 * recognised by the presence of the symbols.
 * So were the sampled transforms with the signs of a seed (fewbit_hipx_sampled_signs, _sampled_dct_signed, _sampled_dft_signed): inside
 * revision 2, recognised by the presence of the symbols.
 * So was the packed form of a seed (fewbit_hipx_quant_bytes, _quant_pack_host, _quant_unpack_host, _quant_pack, _quant_unpack): inside
 * revision 2, recognised by the presence of the symbols.
 * So were the normalized rows of a seed (fewbit_hipx_norm_state_bytes, _norm_workspace, _norm_state_host, _norm_state_unpack_host,
 * _layer_norm_forward, _layer_norm_backward): inside revision 2, recognised by the presence of the symbols.
 * So were the un-centred rows, the RMS norm of the same state (fewbit_hipx_rms_norm_forward, _rms_norm_backward): inside revision 2, recognised by
 * the presence of the symbols.
 * So was the sum of a seed in front of the norm (fewbit_hipx_add_layer_norm_forward, _add_layer_norm_backward, _add_rms_norm_forward,
 * _add_rms_norm_backward): inside revision 2, recognised by the presence of the symbols.
 * So were the gate and the up of a seed, the product of a gated MLP (fewbit_hipx_glu_state_bytes, _glu_state_host, _glu_forward, _glu_backward):
 * inside revision 2, recognised by the presence of the symbols.
 * So was the backward of that product that also rebuilds the product from the state (fewbit_hipx_glu_backward_product, what the gated MLP as one
 * node needs): inside revision 2, recognised by the presence of the symbol.
 * So was the loss of a row, the cross entropy that keeps the logits as given and one float per row (fewbit_hipx_cross_entropy_host,
 * _cross_entropy_forward, _cross_entropy_backward): inside revision 2, recognised by the presence of the symbols. */
#define FEWBIT_HIPX_ABI_VERSION 1
#define FEWBIT_HIPX_REVISION 2

int fewbit_hipx_abi_version(void);
int fewbit_hipx_revision(void);
const char *fewbit_hipx_last_error(void);

/* ------------------------------------------------------------------------------------------------------------------
 * Sampled Fourier transform of the randomized linear layers:
 *     out[0][j][c] + i out[1][j][c] = scale * (1 / sqrt(rows)) * sum_n m[n][c] exp(-2 pi i n idx[j] / rows)
 *   = torch.fft.fft(m, dim=0, norm='ortho')[idx] * scale, the layer's torch.fft formulation, which builds the whole complex
 *     rows x features transform before it gathers the sampled rows
 *   m    rows x features, row-major with leading dimension `ld` (elements), dtype F32 / F16 / BF16; rows = 2^k in [256, 262144],
 *        3 x 2^k in [768, 49152], 5 x 2^k in [1280, 40960], 7 x 2^k in [3584, 57344], 9 x 2^k in [2304, 36864] or 15 x 2^k in
 *        [3840, 30720], the row counts of fewbit_hip_sampled_dct (anything else:
 *        FEWBIT_ERR_UNSUPPORTED, and fewbit_hipx_sampled_dft_workspace returns 0); arithmetic and the intermediate are fp32
 *   idx  proj row numbers in [0, rows) as int64 in DEVICE memory (drawn with replacement: duplicates are served one by one; as in
 *        fewbit_hip_sampled_dct, the low 32 bits of an entry are reduced to [0, rows))
 *   out  two planes of proj x features, contiguous, one after the other: out[0] the real part, out[1] the imaginary part, in
 *        `out_dtype` = FEWBIT_F32 or the dtype of m (fully written)
 *   workspace  fewbit_hipx_sampled_dft_workspace(...) bytes, 16-byte aligned: the formula of fewbit_hip_sampled_dct_workspace
 *        (ceil(features / 64) * rows * 256 + 2048 + 8 * proj rounded up to 16); contents are scratch
 * Exact: rows k = 0 and k = rows / 2 have an imaginary part of 0; a sampled pair k, rows - k gives exact conjugates; the same
 * arguments give the same bits.  Two launches on `stream` (fewbit_amd/csrc/fewbit_dft.hip).
 * Tiles at 32768 rows and more need more than 64 KiB of LDS: the first call of a dtype on a device reserves it for every row
 * count of that dtype, so one eager call per dtype and device precedes a hipGraph capture of any row count of it. */
size_t fewbit_hipx_sampled_dft_workspace(int dtype, size_t rows, size_t features, size_t proj);
int fewbit_hipx_sampled_dft(int dtype, const void *m, size_t rows, size_t features, size_t ld, const int64_t *idx, size_t proj, double scale,
                            int out_dtype, void *out, void *workspace, size_t workspace_bytes, void *stream);
/* The same with the sampled rows a FUNCTION of a 64-bit seed: exactly fewbit_hip_sampled_rows(seed, rows, proj), the rows
 * fewbit_hip_sampled_dct_seeded samples (definition: fewbit_hip.h).  seed_device != NULL: the seed is read from that 8-byte
 * aligned DEVICE word when the kernel runs (`seed` is ignored) -- a launch recorded in a hipGraph then draws fresh rows on every
 * replay, fed by fewbit_hip_sketch_next_seed. */
int fewbit_hipx_sampled_dft_seeded(int dtype, const void *m, size_t rows, size_t features, size_t ld, uint64_t seed, const uint64_t *seed_device,
                                   size_t proj, double scale, int out_dtype, void *out, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The sampled transforms at ANY row count, by zero extension.  m holds valid_rows rows and is transformed as if it had `rows` rows, the
 * missing ones zero:
 *     out = scale * transform_of_length_rows([m; 0])[idx]          transform: the orthonormal DCT-II (fewbit_hip_sampled_dct) or the DFT above
 *   rows        a supported row count (the list above) -- fewbit_hipx_sampled_rows_ceil(n): the smallest one >= n, 256 for n = 1 .. 256,
 *               0 for n = 0 and n > 262144 (from the table the kernels are dispatched by)
 *   valid_rows  1 <= valid_rows <= rows (else FEWBIT_ERR_INVALID_ARGUMENT).  m: valid_rows x features with leading dimension ld; no
 *               address at or beyond m + valid_rows * ld elements is read -- the missing rows are zeros that are never loaded, there is no
 *               padded copy.  valid_rows * ld elements must span less than 4 GiB (else FEWBIT_ERR_UNSUPPORTED)
 *   idx / seed  row numbers in [0, rows) -- of the seed: fewbit_hip_sampled_rows(seed, rows, proj) -- by the rules of the plain entry points
 *   out, out_dtype, scale, stream, the seed word   as in fewbit_hip_sampled_dct[_seeded] (the DCT: no out_dtype, one plane in the dtype of m)
 *               and fewbit_hipx_sampled_dft[_seeded]
 *   workspace   fewbit_hipx_sampled_dft_workspace(dtype, rows, features, proj) bytes (the one formula of all sampled transforms, at `rows`)
 * The result is bit for bit that of the plain entry point on a rows x features copy of m filled up with zeros (valid_rows = rows: on m itself).
 * What it is for: with R sampling p of `rows` rows uniformly with replacement, C the orthonormal transform of length `rows` and P the
 * rows x valid_rows matrix that appends the zero rows, S = sqrt(rows / p) R C P has E[S^T S] = P^T C^T C P = P^T P = I, so (S G)^T (S X)
 * with the same R is an unbiased estimate of G^T X for matrices of valid_rows rows -- an estimator of the same kind as the layer's, but
 * NOT the reference's dct(X)[idx] at length valid_rows: another random variable with the same mean.
 * Pass A skips the missing rows (fewbit_amd/csrc/fewbit_fft4.h: pass_a_zext_kernel); pass B (pass_b_kernel) and the LDS note above are the plain pair's. */
size_t fewbit_hipx_sampled_rows_ceil(size_t rows);
int fewbit_hipx_sampled_dct_zext(int dtype, const void *m, size_t rows, size_t valid_rows, size_t features, size_t ld, const int64_t *idx, size_t proj,
                                 double scale, void *out, void *workspace, size_t workspace_bytes, void *stream);
int fewbit_hipx_sampled_dct_zext_seeded(int dtype, const void *m, size_t rows, size_t valid_rows, size_t features, size_t ld, uint64_t seed,
                                        const uint64_t *seed_device, size_t proj, double scale, void *out, void *workspace, size_t workspace_bytes,
                                        void *stream);
int fewbit_hipx_sampled_dft_zext(int dtype, const void *m, size_t rows, size_t valid_rows, size_t features, size_t ld, const int64_t *idx, size_t proj,
                                 double scale, int out_dtype, void *out, void *workspace, size_t workspace_bytes, void *stream);
int fewbit_hipx_sampled_dft_zext_seeded(int dtype, const void *m, size_t rows, size_t valid_rows, size_t features, size_t ld, uint64_t seed,
                                        const uint64_t *seed_device, size_t proj, double scale, int out_dtype, void *out, void *workspace,
                                        size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The sampled transforms behind a random sign per row: the subsampled RANDOMIZED transform.
 *     out = scale * transform_of_length_rows([D m; 0])[rows of the seed]          D = diag(+-1), valid_rows x valid_rows, of the same seed
 *
 * The signs of a seed.  The sign of matrix row r (the row of m in memory, before any reordering) is a pure function of (seed, r):
 *     w[0..3] = Philox4x32-10(counter = (low 32 bits of r >> 7, high 32 bits of r >> 7, 0, 6), key = (low 32 bits of seed, high 32 bits of seed))
 *               (fewbit_philox.h; counter word 3 = 6 is this domain's own: 0 and 2 are the dense sketches', 3 the sampled rows', 4 the CRS
 *               columns', 5 the dropout's)
 *     flip(r) = bit (r & 31) of w[(r >> 5) & 3]                  1: the row is negated
 * The sampled rows stay fewbit_hip_sampled_rows(seed, rows, proj): one seed serves both.
 *
 * Why.  With R sampling p of `rows` rows uniformly and T the orthonormal transform, S = sqrt(rows / p) R T D has E[S^T S] = D T^H T D = I
 * for EVERY D: the estimate (S G)^T (S X) stays unbiased.  Its variance, summed over entries, is
 * (1 / p) [rows * sum_k |(T D G)_k|^2 |(T D X)_k|^2 - |G^T X|_F^2]: without D whatever many rows of X share (a mean activation, a repeated
 * token) lands in a few rows of T X and the first term grows like `rows` times |G|^2 |X|^2; with D it stays within a small constant of it
 * (at most 3 for a rank-one input under the real transform, 2 under the complex one), the level fewbit_amd.VarianceEstimator's var_rmm assumes.
 *
 * fewbit_hipx_sampled_signs: flip(first + i) for i < count as bytes of 0 / 1 at a HOST pointer; no device is touched; any `first`.
 * fewbit_hipx_sampled_dct_signed / _dft_signed: the arguments, the refusals (with these names in the message) and the workspace of
 *   fewbit_hipx_sampled_dct_zext_seeded / _dft_zext_seeded; valid_rows == rows is the plain case.  seed_device != NULL: the seed word is read
 *   when the kernel runs, for the rows and the signs alike -- a launch recorded in a hipGraph draws fresh rows AND fresh signs on every
 *   replay.  Seeded only: there is no form with an array of row numbers.
 * The result is bit for bit that of the _zext_seeded entry point on a copy of m whose flipped rows are negated (negation is exact in all
 * three dtypes): pass A XORs the sign bits into the 16-byte pieces it has just loaded, before they are widened to fp32 (fewbit_fft4.h:
 * pass_a_zext_kernel with the signs of the seed; fewbit_amd/csrc/fewbit_signed.hip).  Rows that are not loaded, and the zeros a ragged last
 * column tile is filled up with, stay +0.  Pass B, the workspace layout and the LDS note of the plain pair are unchanged; the first signed
 * call of a dtype on a device reserves the LDS of its kernels (one eager call per dtype and device before a hipGraph capture). */
int fewbit_hipx_sampled_signs(uint64_t seed, uint64_t first, size_t count, uint8_t *flip_host);
int fewbit_hipx_sampled_dct_signed(int dtype, const void *m, size_t rows, size_t valid_rows, size_t features, size_t ld, uint64_t seed,
                                   const uint64_t *seed_device, size_t proj, double scale, void *out, void *workspace, size_t workspace_bytes,
                                   void *stream);
int fewbit_hipx_sampled_dft_signed(int dtype, const void *m, size_t rows, size_t valid_rows, size_t features, size_t ld, uint64_t seed,
                                   const uint64_t *seed_device, size_t proj, double scale, int out_dtype, void *out, void *workspace,
                                   size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Column sampling of the weight gradient (LinearCRS; the reference's linear_crs, fewbit/functional/linear.py:27-43): `nopairs`
 * draws with replacement from the in_features columns of the layer's input; the drawn columns are kept, each scaled by
 * count * in_features / nopairs, which makes G^T kept an unbiased estimate of the drawn columns of dL/dW.
 *
 * The columns of a seed.  The draws are a pure function of (seed, in_features, nopairs):
 *     block q = Philox4x32-10(counter = (q, 0, 0, 4), key = (low 32 bits of seed, high 32 bits of seed))      (fewbit_philox.h;
 *               counter word 3 = 4 is this domain's own: 0 and 2 are the dense sketches', 3 the sampled rows')
 *     draw i  = (uint64(word i % 4 of block i / 4) * in_features) >> 32,    i = 0 .. nopairs - 1
 *     cols[0 .. m)  the distinct drawn columns in ASCENDING order,  count[j] = how often cols[j] was drawn  (sum of count = nopairs)
 *     scale[j] = (float)((double)count[j] * in_features / nopairs)
 *     pos[c]   = j if cols[j] == c, else -1,    c = 0 .. in_features - 1
 * Supported: in_features in [1, 2^20], nopairs in [1, 2^22], dtype F32 / F16 / BF16, at least one row; anything else has no kernel
 * (the workspace query returns 0, the entry points FEWBIT_ERR_UNSUPPORTED or FEWBIT_ERR_INVALID_ARGUMENT).
 *
 * fewbit_hipx_crs_columns evaluates the definition on the HOST, with HOST pointers (the counterpart of fewbit_hip_sampled_rows): *m
 * is set, and with cols_host != NULL (then count_host != NULL too, room for min(nopairs, in_features) entries each) the columns and
 * their counts are written.  No device is touched.
 *
 * fewbit_hipx_crs_workspace: bytes of scratch of the two calls below (16-byte aligned; 16 + 4 in_features + 8 min(nopairs, in_features),
 * each part rounded up to 16), 0 = no kernel.  The kernels leave m, pos, cols and scale there; the layout is private.
 *
 * fewbit_hipx_crs_gather: out[r][j] = round_to_dtype(float(x[r][cols[j]]) * scale[j]) for j < m and exactly 0 for m <= j < cap.
 *   x    rows x in_features, row-major with leading dimension `ld` (elements)
 *   seed, seed_device   as in fewbit_hipx_sampled_dft_seeded: seed_device != NULL is an 8-byte aligned DEVICE word read when the
 *        kernel runs (`seed` is ignored), so a launch recorded in a hipGraph draws fresh columns on every replay
 *   cap  columns of `out`, 1 <= cap <= min(nopairs, in_features).  A caller that knows m (from fewbit_hipx_crs_columns) passes it;
 *        one that cannot (the seed is a device word) passes min(nopairs, in_features) >= m.  m is never read back.  (cap < m: only
 *        the first cap columns are written.)
 *   out  rows x cap, contiguous, fully written
 * fewbit_hipx_crs_scatter: gw[o][c] = pos[c] >= 0 ? t[o][pos[c]] : +0 -- ALL of gw (out_features x in_features, contiguous) in one
 * pass, the bits of t copied.  t: the out_features x cap product G^T kept, contiguous; (seed, in_features, nopairs) those of the gather
 * (columns at positions >= cap read as 0).
 * Each call is two launches on `stream` (fewbit_amd/csrc/fewbit_crs.hip): one workgroup that evaluates the definition into the
 * workspace, and the pass over the rows.  The same arguments give the same bits. */
int fewbit_hipx_crs_columns(uint64_t seed, size_t in_features, size_t nopairs, int64_t *cols_host, int32_t *count_host, size_t *m);
size_t fewbit_hipx_crs_workspace(int dtype, size_t rows, size_t in_features, size_t nopairs);
int fewbit_hipx_crs_gather(int dtype, const void *x, size_t rows, size_t in_features, size_t ld, uint64_t seed, const uint64_t *seed_device, size_t nopairs,
                           size_t cap, void *out, void *workspace, size_t workspace_bytes, void *stream);
int fewbit_hipx_crs_scatter(int dtype, const void *t, size_t out_features, size_t cap, uint64_t seed, const uint64_t *seed_device, size_t in_features,
                            size_t nopairs, void *gw, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The moments of the variance estimator (fewbit_amd/variance.py; arXiv:2201.13195, section 3).  For a linear layer's input rows X
 * (rows x n) and output-gradient rows G (rows x m):
 *     fewbit_hipx_row_moments   out3[0] = sx  = sum_b |x_b|^2      out3[1] = sg = sum_b |g_b|^2      out3[2] = sxg = sum_b |x_b|^2 |g_b|^2
 *     fewbit_hipx_sum_squares   out1[0] = sum_i t[i]^2             (on the fp32 product X^T G: cross = |X^T G|_F^2)
 * from which corr = cross / (sx sg), var_sgd = rows / (rows - 1) sxg - cross / (rows - 1), var_rmm = (sx sg - cross) / proj.
 *   x, g   row-major with leading dimensions ldx >= n, ldg >= m (elements); dtype_x and dtype_g are INDEPENDENT, each F32 / F16 / BF16
 *          (under autocast the gradient's dtype differs from the input's); pointers aligned to their element size, nothing more
 *   t      `count` contiguous elements of `dtype`
 *   out3 / out1   3 / 1 doubles in DEVICE memory, 8-byte aligned, written by the second launch
 *   workspace     fewbit_hipx_moments_workspace(rows, n, m) bytes, 16-byte aligned -- for fewbit_hipx_sum_squares:
 *          fewbit_hipx_moments_workspace(count, 1, 1); 24576 today, whatever the extents.  Contents are scratch and need no initialisation
 *   Supported: rows, count, ldx, ldg in [1, 2^31], n and m in [1, 2^24].  A zero or larger extent and ld < n: FEWBIT_ERR_UNSUPPORTED with the
 *          offending value in the message (the workspace query returns 0); an unknown dtype, a null or misaligned pointer and a short
 *          workspace: FEWBIT_ERR_INVALID_ARGUMENT.
 * Arithmetic: every element is widened to fp64 and squared exactly; every sum -- over a row, the product of the two row sums, over the
 * rows -- is accumulated in fp64.  Nothing overflows for finite input (bf16 3e38 included); each output is within (terms added) x 2^-53
 * relative of the exact value and exact whenever every partial sum is representable; NaN and Inf propagate to the outputs they belong to.
 * Order: rows are dealt to waves, a wave reduces a row in a fixed lane order, a workgroup writes its three sums to the workspace, and a
 * second launch of one workgroup adds those partials in a fixed order (lane l the partials l, l + 64, .. ascending, then a fixed
 * butterfly).  There are no floating-point atomics: the same arguments give the same bits.  The plan is a pure function of the row count:
 * rows per workgroup = max(16, ceil(rows / 1024)), at most 1024 workgroups (sum_squares: pieces of 1024 elements as rows, at least 4 per
 * workgroup).
 * Reads: each element of X, G and t once, 16 bytes at a time wherever a row's 16-byte aligned interior allows and element by element at
 * its head and tail; no address at or beyond x + rows * ldx or g + rows * ldg and no element of a row's padding [n, ldx) is read.
 * Two launches per call on `stream` (fewbit_amd/csrc/fewbit_moments.hip), no synchronisation: both calls can be captured into a hipGraph. */
size_t fewbit_hipx_moments_workspace(size_t rows, size_t n, size_t m);
int fewbit_hipx_row_moments(int dtype_x, const void *x, size_t n, size_t ldx, int dtype_g, const void *g, size_t m, size_t ldg, size_t rows, double *out3,
                            void *workspace, size_t workspace_bytes, void *stream);
int fewbit_hipx_sum_squares(int dtype, const void *t, size_t count, double *out1, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Dropout that keeps nothing for backward: the mask is a pure function of (seed, threshold, element index), evaluated alike by the
 * host function and the kernel, so backward regenerates it from the seed.
 *
 * The mask of a seed.  For the element at flat index i of a logical contiguous tensor:
 *     q       = i >> 3
 *     w[0..3] = Philox4x32-10(counter = (low 32 bits of q, high 32 bits of q, 0, 5), key = (low 32 bits of seed, high 32 bits of seed))
 *               (fewbit_philox.h; counter word 3 = 5 is this domain's own: 0 and 2 are the dense sketches', 3 the sampled rows', 4 the
 *               CRS columns')
 *     u(i)    = 16 bits of the block: word (i & 7) >> 1, its LOW half for even i, its HIGH half for odd i
 *     T       = the threshold: the nearest integer to p * 65536 (ties to even), 0 <= T <= 65536
 *     keep(i) = u(i) >= T                                   P(drop) = T / 65536 exactly
 *     scale   = (float)(65536.0 / (65536 - T))              (T = 65536: everything is dropped, the scale is not used)
 *     out[i]  = keep(i) ? round_to_dtype(float(src[i]) * scale [+ float(addend[i])]) : (addend ? addend[i] : +0)
 * The product and the sum are separate fp32 operations and the result is rounded once to the dtype.  A dropped element is exactly +0 (with an
 * addend: the addend's bits) whatever src holds -- an inf or NaN there has no influence on the result.  The scale is that of the realized
 * probability T / 65536, so E[out] = src [+ addend] exactly; |p - T / 65536| <= 2^-17.
 *
 * fewbit_hipx_dropout_threshold: T of p on the host, -1 for p outside [0, 1] or NaN.
 * fewbit_hipx_dropout_keep: keep(first + j) for j < count as bytes of 0 / 1 at a HOST pointer; no device is touched; any `first`
 *   (threshold > 65536: FEWBIT_ERR_INVALID_ARGUMENT).
 * fewbit_hipx_dropout: ONE launch on `stream` (fewbit_amd/csrc/fewbit_dropout.hip); forward (src = x) and backward (src = gy, addend = NULL) alike.
 *   dtype        F32 / F16 / BF16, of src, addend and out; n elements each, contiguous
 *   first        the flat index of src[0] in the logical tensor, a multiple of 8: a shard of a tensor draws the mask of the whole tensor
 *   addend       may be NULL; given, out = addend + dropout(src) in the same pass
 *   out          may alias src exactly, or addend exactly (any other overlap is undefined)
 *   seed, seed_device   as in fewbit_hipx_crs_gather: seed_device != NULL is an 8-byte aligned DEVICE word read when the kernel runs (`seed`
 *                is ignored), so a launch recorded in a hipGraph draws a fresh mask on every replay
 *   threshold    T, 0 .. 65536
 * Pointers need only the alignment of their element.  With src, addend and out all 16-byte aligned one Philox call serves eight elements
 * moved by 16-byte loads and stores (one per lane for the 16-bit types, two for fp32); otherwise the elements are moved one by one and the
 * bytes are the same.  No address at or beyond n elements is read or written.  No LDS, no workspace, no atomics: the same arguments give the
 * same bits.  The plan is a pure function of n: lanes take blocks of 8 elements, 256 lanes to a workgroup, at most 2048 workgroups (2^22
 * elements), beyond which each lane sweeps on by the width of the grid.
 * Refused before anything is launched (FEWBIT_ERR_INVALID_ARGUMENT): an unknown dtype, threshold > 65536, first not a multiple of 8, a
 * misaligned seed word, a null src or out, a pointer not aligned to its element.  n = 0: FEWBIT_OK, no launch. */
int fewbit_hipx_dropout_threshold(double p);
int fewbit_hipx_dropout_keep(uint64_t seed, uint32_t threshold, uint64_t first, size_t count, uint8_t *keep_host);
int fewbit_hipx_dropout(int dtype, const void *src, const void *addend, void *out, size_t n, uint64_t first, uint64_t seed, const uint64_t *seed_device,
                        uint32_t threshold, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * A tensor kept in 2, 4 or 8 bits per element with unbiased stochastic rounding (what QuantizedLinear keeps of its input): the packed
 * buffer is a pure function of (values, bits, seed), evaluated alike by the host function and the kernel.
 *
 * The packed form of a seed.  The input is a logical contiguous tensor of n elements (F32 / F16 / BF16), each widened exactly to fp32;
 * bits = k in {2, 4, 8}, L = 2^k - 1; a 64-bit seed.  Elements are taken by flat index i; group g is the elements 64 g .. min(64 g + 64, n) - 1
 * (groups may straddle the rows of a matrix).
 *     u(i)    = the 16 bits the mask of a seed (above) takes for index i -- the same block q = i >> 3, word and half -- with counter word 3 = 7
 *               (this domain's own: 0 and 2 to 6 are taken)
 *     U(i)    = float(u(i)) / 65536                                         (exact)
 *   per group:
 *     lo, hi  = the minimum and the maximum of the group's elements (exact; -0 counts as below +0, so both are defined to the bit)
 *     range   = hi - lo                                                     (one fp32 subtraction)
 *     poisoned: an element is NaN or +-inf, or range is not finite.  Then lo = step = NaN (the canonical quiet NaN 0x7fc00000) and every
 *               code is 0; every element of the group decodes to that NaN; other groups are untouched.
 *     otherwise step = range / L and inv = range > 0 ? L / range : 0 (each ONE correctly rounded fp32 division); where L / range overflows
 *               (range < L / FLT_MAX, about 7.5e-37 at 8 bits) inv = 0 as well: every element of such a group decodes to lo, within range.
 *   per element:
 *     t       = (x - lo) * inv                                              (two separate fp32 operations, never contracted)
 *     code    = min(L, (uint)floor(t + U(i)))                               (one fp32 addition)
 *     decode  = fma(float(code), step, lo), rounded once to the output dtype (a poisoned group: the canonical quiet NaN of that dtype)
 * Hence |decode - x| <= step up to fp32 rounding, E[decode] = x up to the 2^-16 granularity of U, and a constant group decodes exactly.
 *
 * The buffer: fewbit_hipx_quant_bytes(n, k) = 8 ceil(n / 64) + k ceil(n / 8) bytes.  First the parameters, per group lo then step as fp32
 * little-endian; then the codes, per 8 consecutive elements one little-endian word of k bytes with element j in bits [k j, k j + k).  The
 * missing elements of the last word are 0.  The same arguments give the same bytes; the buffer does not depend on the source dtype beyond
 * the values.
 *
 * fewbit_hipx_quant_bytes: the size above; 0 for bits other than 2, 4, 8 and for n outside 1 .. 2^36.
 * fewbit_hipx_quant_pack_host / _unpack_host: the definition and the fp32 decode at HOST pointers; no device is touched.
 * fewbit_hipx_quant_pack: ONE launch on `stream` (fewbit_amd/csrc/fewbit_quant.hip).
 *   dtype, src   F32 / F16 / BF16; n elements, contiguous, aligned to the element.  With src 16-byte aligned a lane takes its 8 elements by
 *                16-byte loads (one for the 16-bit types, two for fp32), otherwise and in the block that holds the tail element by element:
 *                the same bytes either way.  No address at or beyond n elements is read.
 *   seed, seed_device   as in fewbit_hipx_dropout: seed_device != NULL is an 8-byte aligned DEVICE word read when the kernel runs (`seed` is
 *                ignored), so a launch recorded in a hipGraph rounds afresh on every replay
 *   out, out_bytes   8-byte aligned, at least fewbit_hipx_quant_bytes(n, bits) bytes; nothing beyond that many bytes is written
 * fewbit_hipx_quant_unpack: ONE launch on `stream`.
 *   packed       the buffer of a pack call of the same n and bits, 8-byte aligned
 *   out_dtype, out   F32 / F16 / BF16, independent of the dtype that was packed (under autocast a gradient's dtype differs from the input's);
 *                n elements, aligned to the element; 16-byte stores where out is 16-byte aligned, element stores otherwise and in the tail
 * No LDS, no workspace, no atomics, no read-back: the same arguments give the same bits.  The plan is a pure function of n: lanes take blocks
 * of 8 elements, 8 neighbouring lanes hold a group (its minimum, maximum and poison flag are reduced across them by DPP lane moves, not through LDS), 256 lanes
 * to a workgroup, at most 2048 workgroups (2^22 elements), beyond which each lane sweeps on by the width of the grid.
 * Refused before anything is launched (FEWBIT_ERR_INVALID_ARGUMENT): an unknown dtype, bits other than 2, 4, 8, n beyond 2^36, a null or
 * misaligned pointer, out_bytes below the size, a misaligned seed word.  n = 0: FEWBIT_OK, no launch. */
size_t fewbit_hipx_quant_bytes(size_t n, int bits);
int fewbit_hipx_quant_pack_host(const float *x_host, size_t n, int bits, uint64_t seed, uint8_t *out_host);
int fewbit_hipx_quant_unpack_host(const uint8_t *packed_host, size_t n, int bits, float *out_host);
int fewbit_hipx_quant_pack(int dtype, const void *src, size_t n, int bits, uint64_t seed, const uint64_t *seed_device, uint8_t *out, size_t out_bytes,
                           void *stream);
int fewbit_hipx_quant_unpack(const uint8_t *packed, size_t n, int bits, int out_dtype, void *out, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * A layer norm that keeps its NORMALIZED input in 2, 4 or 8 bits per element for backward (what QuantizedLayerNorm keeps instead of its input):
 * the state is a pure function of (x^, bits, seed), evaluated alike by the host function and the kernel.
 *
 * The normalized rows of a seed.  The input is a contiguous rows x width matrix (F32 / F16 / BF16), each element widened exactly to fp32.
 *   Row statistics, per row r, every step ONE fp32 operation:
 *     mean    = (the sum of the row) / width
 *     var     = (the sum of (x - mean)^2) / width     two passes over the row the lanes already hold -- not E[x^2] - mean^2, which cancels
 *               for a row such as 1000 + noise.  The order of the two sums is the kernel's (fewbit_amd/csrc/fewbit_norm.hip); what the state
 *               is a function of is x^, which fewbit_hipx_layer_norm_forward hands out on request (xhat_out).
 *     rstd    = 1 / sqrt(var + float32(eps))           (an addition, a square root, a division)
 *     x^      = (x - mean) * rstd
 *     y       = round_to_dtype(x^ * gamma + beta)      a product and a sum in fp32, rounded once.  gamma and beta are read in the dtype of x and
 *               widened exactly; a NULL gamma counts as 1 and a NULL beta as 0.
 *   Groups and blocks are PER ROW: B = ceil(width / 8) blocks and G = ceil(width / 64) groups to a row; the last block and the last group of a
 *     row may be short.  Missing elements count for neither the minimum nor the maximum and their codes are 0 (the rule of the tail of a
 *     tensor in the packed form of a seed).
 *   Codes: lo, step, inv, code, decode and the poison rule are those of the packed form of a seed (above; one text, fewbit_quantdef.h).  The 16
 *     rounding bits of element 8 b + e of row r are those the packed form takes for element e of block q = r * B + b (a 64-bit value), counter
 *     word 3 = 7.
 *   The state, fewbit_hipx_norm_state_bytes(rows, width, k) = rows * (8 G + C) bytes with C = k * B rounded up to a multiple of 4:
 *     first the (lo, step) pairs, fp32 little-endian, ordered (r, g): 8 * rows * G bytes;
 *     then the codes: row r starts at 8 * rows * G + r * C, block b of it is a little-endian word of k bytes at k * b with element j in bits
 *     [k j, k j + k); the bytes of a row behind its last block (two of them, at 2 bits and an odd B) are 0.
 *     For width % 64 == 0 the state is byte for byte fewbit_hipx_quant_pack_host of the flat x^ with the same seed and bits.
 *   Backward, fp32 throughout, every step ONE operation:
 *     x^q = decode(state), g^ = gy * gamma
 *     dx  = round_to_dtype(rstd * ((g^ - mean_row(g^)) - x^q * mean_row(g^ * x^q)))              mean_row: (the sum of the row) / width
 *     dgamma = sum_r gy * x^q,  dbeta = sum_r gy                                                   as fp32
 *   NaN and infinity: a non-finite element (or a row whose fp32 sum overflows) makes its row's x^ and y NaN and poisons every group of the
 *     row; that row of dx and the columns of dgamma it touches are then NaN, as with torch.  Other rows are untouched to the bit.  A finite
 *     row whose sum stays finite while the fp32 sum of its centred squares overflows (alternating +-2^66 at an even width: the sum is exactly
 *     0) gives var = inf, rstd = 0, x^ = +-0 and y = beta; no group is poisoned, and that row of dx is +-0.
 *   Since E[x^q] = x^, dgamma is unbiased.  dx is not exactly: x^q enters it twice, E[dx_q] - dx = -rstd * g^_i * Var(x^q_i) / width, second
 *     order in the step.
 *
 * The un-centred rows (the RMS norm: what QuantizedRMSNorm keeps).  The same input, every step again ONE fp32 operation, contraction off:
 *     ms      = (the sum of x * x over the row) / width
 *     rstd    = 1 / sqrt(ms + float32(eps))            (an addition, a square root, a division)
 *     x^      = x * rstd
 *     y       = round_to_dtype(x^ * gamma)             gamma in the dtype of x, widened exactly; NULL counts as 1; rounded once
 *     state   = the state of the normalized rows of a seed for these x^: the same groups per row, rounding bits, layout and size
 *               fewbit_hipx_norm_state_bytes(rows, width, bits); fewbit_hipx_norm_state_host / _unpack_host serve both norms (the state is a
 *               function of x^ only)
 *   Backward, fp32, one operation per step:
 *     x^q = decode(state), g^ = gy * gamma
 *     dx  = round_to_dtype(rstd * (g^ - x^q * mean_row(g^ * x^q)))
 *     dgamma = sum_r gy * x^q                                                                      as fp32
 *   The order of a row sum is the kernel's, that of the layer norm; the per-workgroup partials of dgamma are added in the same fixed order.
 *   Since E[x^q] = x^, dgamma is unbiased; E[dx_q] - dx = -rstd * g^_i * Var(x^q_i) / width, second order in the step, as for the layer norm.
 *   NaN and infinity are what the fp32 arithmetic gives, and what torch's own formulation gives.  A NaN element makes its row of x^, y and dx NaN,
 *     poisons every group of the row and makes dgamma NaN in every column.  An INFINITE element makes ms infinite, so rstd is 0 and x^ is NaN at
 *     that element and +-0 elsewhere: the group that holds the NaN is poisoned by the rule of the packed form, dx of that row is NaN (the row
 *     mean is), dgamma is NaN in that group's columns.  Other rows are untouched to the bit.  A finite row whose fp32 sum of squares overflows
 *     (bf16 values near 1e20) gives rstd = 0 and x^ = y = +-0.
 *
 * fewbit_hipx_norm_state_bytes: the size above; 0 for bits other than 2, 4, 8, width outside 1 .. 8192, rows = 0 and rows * width beyond 2^36.
 * fewbit_hipx_norm_workspace: bytes of scratch of fewbit_hipx_layer_norm_backward (16-byte aligned; the per-workgroup partial sums of dgamma and
 *   dbeta; contents are scratch); 0 for the same shapes.
 * fewbit_hipx_norm_state_host / _unpack_host: the state of given fp32 x^ (rows x width, contiguous) and its fp32 decode (rows x width) at HOST
 *   pointers; no device is touched.
 * fewbit_hipx_layer_norm_forward: ONE launch on `stream`.
 *   dtype, x, y, gamma, beta   F32 / F16 / BF16; aligned to the element; gamma and beta may be NULL.  A row is loaded once, by 16-byte accesses
 *                where its base is 16-byte aligned and element by element otherwise and in its ragged tail: the same bytes either way
 *   seed, seed_device   as in fewbit_hipx_quant_pack: seed_device != NULL is an 8-byte aligned DEVICE word read when the kernel runs
 *   rstd         rows fp32; required with a state
 *   state, state_bytes   8-byte aligned, at least fewbit_hipx_norm_state_bytes bytes; nothing beyond that many is written.  state == NULL: the
 *                plain forward that keeps nothing (bits and the seed are ignored; rstd may be NULL too); y and rstd are the same bytes
 *   xhat_out     NULL, or rows x width fp32 that receive the x^ the kernel quantized (the seam at which a test meets the host function)
 * fewbit_hipx_layer_norm_backward: TWO launches on `stream`: dx and per-workgroup partial sums, then the partials added in a fixed order.
 *   gy, dx, gamma   of `dtype`; dgamma, dbeta: width fp32.  dx, dgamma, dbeta may each be NULL: that output is skipped and nothing of it
 *                written (both sums NULL: one launch, no workspace needed).  rstd is read for dx only.
 * fewbit_hipx_rms_norm_forward / fewbit_hipx_rms_norm_backward: the un-centred rows by the same kernels with the kind switched at compile time, the
 *   contracts, refusals and alignment rules of the layer-norm pair without beta and dbeta: ONE row sum per tile forward and backward, state == NULL
 *   the plain forward with the same y and rstd bytes, dx or dgamma NULL skipped and untouched, dgamma NULL one launch and no workspace, otherwise the
 *   column sums are launched for dgamma alone.  fewbit_hipx_norm_workspace is the size query for both backwards.
 * Widths 1 .. 8192, rows * width <= 2^36.  The plan is a pure function of (rows, width): a row takes 8, 16, 64, 128 or 256 lanes (widths up to
 * 64, 128, 512, 1024, 2048), a lane one block of 8 elements; beyond 2048 elements a forward lane takes 2 blocks and beyond 4096 four, a backward
 * row 512 and 1024 lanes.  Forward: 256 lanes to a workgroup, at most 16384 workgroups; backward: 1024 lanes, at most 512 workgroups; beyond
 * that a workgroup walks on by the width of the grid.  Sums across lanes go by DPP lane moves inside 16 lanes, v_readlane inside a wave and LDS
 * across the waves of a row, in a fixed order; there are no float atomics and no waiting between workgroups: the same arguments give the same
 * bytes.
 * Refused before anything is launched (FEWBIT_ERR_INVALID_ARGUMENT): an unknown dtype, bits other than 2, 4, 8, a width outside 1 .. 8192,
 * rows * width beyond 2^36, eps negative or not finite, a null or misaligned pointer, a state or workspace that is too small, a misaligned
 * seed word.  rows = 0: FEWBIT_OK, no launch. */
size_t fewbit_hipx_norm_state_bytes(size_t rows, size_t width, int bits);
size_t fewbit_hipx_norm_workspace(size_t rows, size_t width);
int fewbit_hipx_norm_state_host(const float *xhat_host, size_t rows, size_t width, int bits, uint64_t seed, uint8_t *out_host);
int fewbit_hipx_norm_state_unpack_host(const uint8_t *state_host, size_t rows, size_t width, int bits, float *out_host);
int fewbit_hipx_layer_norm_forward(int dtype, const void *x, size_t rows, size_t width, const void *gamma, const void *beta, double eps, int bits, uint64_t seed,
                                   const uint64_t *seed_device, void *y, float *rstd, uint8_t *state, size_t state_bytes, float *xhat_out, void *stream);
int fewbit_hipx_layer_norm_backward(int dtype, const void *gy, const uint8_t *state, const float *rstd, const void *gamma, size_t rows, size_t width, int bits,
                                    void *dx, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, void *stream);
int fewbit_hipx_rms_norm_forward(int dtype, const void *x, size_t rows, size_t width, const void *gamma, double eps, int bits, uint64_t seed,
                                 const uint64_t *seed_device, void *y, float *rstd, uint8_t *state, size_t state_bytes, float *xhat_out, void *stream);
int fewbit_hipx_rms_norm_backward(int dtype, const void *gy, const uint8_t *state, const float *rstd, const void *gamma, size_t rows, size_t width,
                                  int bits, void *dx, float *dgamma, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The sum of a seed in front of the norm: a sublayer's ending, y = norm(residual + dropout(x)), as ONE launch forward and TWO backward (what
 * DropoutAddLayerNorm and DropoutAddRMSNorm run).  ONE seed feeds the mask (counter word 3 = 5) and the rounding bits (counter word 3 = 7).
 * Everything is the existing arithmetic in the existing order, so every output is bit for bit what fewbit_hipx_dropout followed by the plain
 * entry point of the norm gives:
 *     T = threshold (0 .. 65535, in units of 2^-16: fewbit_hipx_dropout_threshold), scale = float32(65536 / (65536 - T))
 *     keep(i) = the mask of the seed at flat index i = r * width + c
 *   forward, per element, fp32:
 *     h       = keep ? round_to_dtype(float(x) * scale + float(residual)) : residual (its bits)        T = 0: every element is kept, nothing is drawn
 *     the norm of the rows of h AS ROUNDED: y, rstd, state and xhat_out are those of the plain forward on h with the same seed
 *     h_out   NULL, or rows x width of `dtype` that receive h (post-norm: nobody else reads the sum, so it never exists in memory)
 *   backward, per element, fp32:
 *     dx32    = what the plain backward rounds to dx
 *     dres    = round_to_dtype(dx32 + float(gh))          gh: NULL, or the gradient arriving at h (pre-norm: h goes on as the residual stream)
 *     dbranch = keep ? round_to_dtype(float(dres) * scale) : +0                                        fewbit_hipx_dropout of dres, no addend
 *     dres is the gradient of the residual, dbranch that of x.  With T = 0 they are the same values: dbranch must be NULL then.
 *     dgamma, dbeta: those of the plain backward (the same partial sums, the same second launch).
 *   dres, dbranch, dgamma and dbeta may each be NULL: that output is skipped and nothing of it is written.
 * The mask is drawn on blocks of eight FLAT elements and a lane holds eight elements of a ROW: with T > 0 the width must be a multiple of 8
 * (anything else: FEWBIT_ERR_UNSUPPORTED; compose the two calls).  With T = 0 every width 1 .. 8192 is served.
 * No output may overlap an input or another output.  The plan, the alignment rules and the refusals are those of the plain pair; refused on top:
 * threshold >= 65536, a NULL residual, residual / h_out / gh / dres / dbranch not aligned to their element, dbranch with T = 0. */
int fewbit_hipx_add_layer_norm_forward(int dtype, const void *x, const void *residual, size_t rows, size_t width, const void *gamma, const void *beta, double eps,
                                       int bits, uint64_t seed, const uint64_t *seed_device, uint32_t threshold, void *y, void *h_out, float *rstd, uint8_t *state,
                                       size_t state_bytes, float *xhat_out, void *stream);
int fewbit_hipx_add_layer_norm_backward(int dtype, const void *gy, const void *gh, const uint8_t *state, const float *rstd, const void *gamma, size_t rows,
                                        size_t width, int bits, uint64_t seed, const uint64_t *seed_device, uint32_t threshold, void *dres, void *dbranch,
                                        float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, void *stream);
int fewbit_hipx_add_rms_norm_forward(int dtype, const void *x, const void *residual, size_t rows, size_t width, const void *gamma, double eps, int bits,
                                     uint64_t seed, const uint64_t *seed_device, uint32_t threshold, void *y, void *h_out, float *rstd, uint8_t *state,
                                     size_t state_bytes, float *xhat_out, void *stream);
int fewbit_hipx_add_rms_norm_backward(int dtype, const void *gy, const void *gh, const uint8_t *state, const float *rstd, const void *gamma, size_t rows, size_t width,
                                      int bits, uint64_t seed, const uint64_t *seed_device, uint32_t threshold, void *dres, void *dbranch, float *dgamma,
                                      void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The product of a gated MLP, y = act(gate) * up (down(act(gate(x)) * up(x)) of the Llama / Mistral / Qwen / Gemma / T5-v1.1 blocks), that keeps
 * BOTH inputs in 2, 4 or 8 bits per element for backward instead of gate, act(gate) and up (what QuantizedGLU keeps): ONE launch forward, ONE
 * backward.  The state is a pure function of (gate, up, bits, seed), evaluated alike by the host function and the kernel.
 *
 * The gate and the up of a seed.  gate and up are logical rows x width matrices of one dtype (F32 / F16 / BF16) with unit stride along the width
 * and row strides ld_gate, ld_up >= width in elements (gate and up may be the two halves of one rows x 2 width matrix: ld = 2 width).  Elements are
 * taken by logical flat index i = r * width + c, n = rows * width; each is widened exactly to fp32.
 *   Forward, per element:
 *     y[i]    = round_to_dtype(act(g) * u)       act evaluated in fp32, then ONE fp32 product, rounded once; y is contiguous (rows x width).
 *               (torch's F.silu(gate) * up rounds act(gate) to the dtype first: a 16-bit y may differ from it in its last bit.)
 *     act     = FEWBIT_SILU: g * sigmoid(g), or FEWBIT_GELU: g * Phi(g), the erf form.  The functors of the activation kernels
 *               (fewbit_amd/csrc/fewbit_device.h): the precise class for fp32 I/O, the fast class for 16-bit I/O.  The tanh form of gelu is not done.
 *               One exception: gelu with 16-bit I/O.  Both classes hold gelu to an error relative to |g|, which below g = -2 is not relative to
 *               gelu(g) (the fast class keeps Phi(-|g|) to 4.5e-8 absolute, the precise class cancels in 1 + erf), and here the value is multiplied
 *               by u and rounded to half an ulp of the PRODUCT.  There g < -1/2 is evaluated as g * 0.5 * erfc(-g / sqrt 2) with the rounding error
 *               of the argument fed back (fewbit_glu.hip, gelu_relative): a few fp32 ulps of gelu(g) on the whole line.
 *               And silu with 16-bit I/O, for the same reason: the fast class's sigmoid rounds its argument once (|g| 2^-24 of the value) and is 0
 *               below g = -87.4, where silu(g) is still a bf16 number down to g = -105.  g * sigmoid(g) is evaluated with the rounding error of
 *               g log2 e fed back and, below g = -64, with the exponent scaled by 2^64 and the scale multiplied in last (sigmoid_relative): a few
 *               fp32 ulps of silu(g), or half an fp32 subnormal, on the whole line.  act' of silu takes the same sigmoid.
 *   The state, fewbit_hipx_glu_state_bytes(n, k) = 2 P bytes with P = fewbit_hipx_quant_bytes(n, k) rounded up to a multiple of 8:
 *     bytes [0, P): the gate part, byte for byte fewbit_hipx_quant_pack_host(gate as a contiguous tensor, n, k, seed) -- flat groups of 64 (they
 *               may straddle rows), counter word 3 = 7 -- then zero bytes up to P;
 *     bytes [P, 2 P): the up part, the same definition of up with counter word 3 = 8 (the next free domain: the two roundings of one seed are
 *               independent), then zero bytes.
 *     fewbit_hipx_quant_unpack_host decodes either part (pass state or state + P).
 *   Backward, fp32, every step ONE operation, never contracted.  With g^ = decode(gate part), u^ = decode(up part):
 *     d_up    = round_to_dtype(gy * act(g^))
 *     d_gate  = round_to_dtype((gy * u^) * act'(g^))
 *     silu:   s = sigmoid(g^), act' = s * (1 + g^ * (1 - s))
 *     gelu:   act' = Phi(g^) + g^ * phi(g^),  Phi = 0.5 * (1 + erf(g^ / sqrt 2)),  phi = exp(-g^ g^ / 2) / sqrt(2 pi)
 *     act and sigmoid are the functors of the forward; gy is contiguous; d_gate and d_up have row strides ld_dgate, ld_dup >= width.
 *   E[g^] = g and E[u^] = u, and the two are independent, but act is not linear: E[act(g^)] - act(g) = act''(g) Var(g^) / 2 + ..., so BOTH gradients
 *     carry a bias of second order in the step (d_up through act, d_gate through act'), as dx of the norms does.  Exactly:
 *     E[d_up] = gy * ((1 - f) act(v0) + f act(v1)) and E[d_gate] = gy * u * ((1 - f) act'(v0) + f act'(v1)), v0 and v1 = v0 + step the two neighbouring
 *     levels of g and f = (g - v0) / step (up to the 2^-16 granularity of U).
 *   NaN and infinity: y is always the exact forward, whatever the groups hold.  A group of EITHER input that holds a NaN or an infinity is poisoned
 *     by the rule of the packed form and decodes to NaN; BOTH gradients are then NaN on the 64 elements of that group, whichever input it was.
 *     Other groups are untouched to the bit.
 *
 * fewbit_hipx_glu_state_bytes: the size above; 0 for bits other than 2, 4, 8 and for n outside 1 .. 2^36.
 * fewbit_hipx_glu_state_host: the state of given fp32 values (n each, contiguous) at HOST pointers; no device is touched.
 * fewbit_hipx_glu_forward: ONE launch on `stream` (fewbit_amd/csrc/fewbit_glu.hip).
 *   gate, up, y  of `dtype`, aligned to the element.  A lane takes a block of 8 flat elements of both inputs by 16-byte accesses where
 *                width % 8 == 0, every row stride times the element size is a multiple of 16 and gate, up and y are 16-byte aligned; element by
 *                element with (r, c) from the flat index otherwise: the same bytes either way.  No address between `width` and a row stride is
 *                touched, none beyond the last row.  y may not overlap gate or up.
 *   seed, seed_device   as in fewbit_hipx_quant_pack: seed_device != NULL is an 8-byte aligned DEVICE word read when the kernel runs (`seed` is
 *                ignored), so a launch recorded in a hipGraph rounds afresh on every replay
 *   state, state_bytes   8-byte aligned, at least fewbit_hipx_glu_state_bytes(n, bits) bytes; nothing beyond that many is written.  state == NULL:
 *                the plain forward that keeps nothing (bits and the seed are ignored); y is the same bytes
 * fewbit_hipx_glu_backward: ONE launch on `stream`.
 *   gy           rows x width of `dtype`, contiguous; state: the buffer of a forward of the same rows, width and bits
 *   d_gate, d_up of `dtype`; either may be NULL: that output is skipped and nothing of it is written (both NULL: no launch).  The 16-byte path
 *                needs width % 8 == 0 and gy and every output present 16-byte aligned with such a row stride.  The gap of a row stride is not written.
 * fewbit_hipx_glu_backward_product: fewbit_hipx_glu_backward with a third output, in the same ONE launch and by the same plan (what the gated MLP
 *                as one node runs: down_proj's weight gradient needs the product y, and nothing of y is kept).
 *   product      rows x width of `dtype`, row stride ld_product >= width:  product[i] = round_to_dtype(act(g^) * u^), the forward's own expression
 *                (the same act, ONE fp32 product, rounded once) evaluated on the decodes.  E[product] = E[act(g^)] * u: the two roundings are
 *                independent, and act is not linear -- a bias of second order in the step, as d_up carries.
 *   d_gate, d_up exactly the arithmetic, and the bytes, of fewbit_hipx_glu_backward.
 *   Any of the three outputs may be NULL: that output is skipped and nothing of it is written (all three NULL: no launch).  gy may be NULL only
 *                where d_gate and d_up both are (only the product is wanted).  A poisoned group is NaN on its 64 elements of all three outputs.
 *   The rules of alignment and stride, the choice between the 16-byte and the element path and the refusals are those of fewbit_hipx_glu_backward
 *                with `product` as one more output; a NULL gy with a gradient wanted is refused.  The gap of a row stride is never written.
 * No LDS, no workspace, no atomics, no read-back: the same arguments give the same bits.  The plan is that of the packed form of a seed: lanes take
 * blocks of 8 elements (of both inputs: two Philox calls, two code words), 8 neighbouring lanes hold a group of each and reduce both minima, maxima
 * and poison flags by DPP lane moves, 256 lanes to a workgroup, at most 2048 workgroups, beyond which each lane sweeps on by the width of the grid.
 * Refused before anything is launched (FEWBIT_ERR_INVALID_ARGUMENT): an unknown dtype, an activation other than FEWBIT_SILU and FEWBIT_GELU, bits
 * other than 2, 4, 8 (with a state), width = 0, rows * width beyond 2^36, a row stride below the width, a null or misaligned pointer, state_bytes
 * below the size, a misaligned seed word.  rows = 0: FEWBIT_OK, no launch. */
size_t fewbit_hipx_glu_state_bytes(size_t n, int bits);
int fewbit_hipx_glu_state_host(const float *gate_host, const float *up_host, size_t n, int bits, uint64_t seed, uint8_t *out_host);
int fewbit_hipx_glu_forward(int dtype, int act, const void *gate, size_t ld_gate, const void *up, size_t ld_up, size_t rows, size_t width, int bits, uint64_t seed,
                            const uint64_t *seed_device, void *y, uint8_t *state, size_t state_bytes, void *stream);
int fewbit_hipx_glu_backward(int dtype, int act, const void *gy, const uint8_t *state, size_t rows, size_t width, int bits, void *d_gate, size_t ld_dgate, void *d_up,
                             size_t ld_dup, void *stream);
int fewbit_hipx_glu_backward_product(int dtype, int act, const void *gy, const uint8_t *state, size_t rows, size_t width, int bits, void *d_gate, size_t ld_dgate,
                                     void *d_up, size_t ld_dup, void *product, size_t ld_product, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The loss of a row: the cross entropy of a row of logits against a class index, F.cross_entropy(x, t, reduction='none') with its gradient,
 * that keeps for backward the logits AS GIVEN and ONE fp32 number per row (what fewbit.CrossEntropyLoss keeps) instead of the log-softmax of every
 * element -- in fp32 where the logits are cast first, as the Hugging Face losses and torch.autocast do.  ONE launch forward, ONE backward.
 *
 * logits is a rows x width matrix of `dtype` (F32 / F16 / BF16) with unit stride along the width and a row stride of ld >= width elements;
 * target holds rows int64 class indices.  Per row, with x the row widened exactly and t its target:
 *     lse       = log sum_j exp(x_j)          evaluated as M + log sum_j exp(x_j - M), M = max_j x_j
 *     loss      = lse - x_t
 *     dlogits_j = grow * (exp(x_j - lse) - [j = t])       rounded ONCE to `dtype`
 *   The host function evaluates this in float64 and is the definition; the kernels evaluate the same in fp32 (fewbit_amd/csrc/fewbit_xent.hip:
 *   exp(a) as v_exp_f32 of a * log2(e), a running maximum and sum per lane rescaled once per block of eight elements, the lanes merged by a
 *   fixed xor butterfly and the four waves in wave order; no floating-point atomics, the same arguments give the same bits).  For |x| <= 16
 *   and V = width, against the host function:
 *     |lse - lse64|   <= E = (V + 128) 2^-24 + 4 2^-24 |lse64|
 *     |loss - loss64| <= E + 4 2^-24 (|lse64| + |x_t|)
 *     |d - d64|       <= |grow| (p64 (E + 160 2^-24) + 2^-23) + r |d64|,  p64 = exp(x_j - lse64),  r = 0 (F32), 2^-11 and 2^-25 absolute
 *                        (F16), 2^-8 (BF16)
 *   Special rows:
 *     t == ignore_index          loss = +0 and every dlogits_j = +0; lse is still written; backward reads nothing of the row
 *     t outside [0, width)       (and not ignore_index) loss = NaN and every dlogits_j = NaN; nothing of the row is read through t, no
 *                                device assertion fires
 *     x_j = -inf                 has probability 0 and dlogits_j = +0 (also for grow < 0)
 *     a NaN or a +inf in the row, or -inf everywhere: loss = NaN and every dlogits_j = NaN (torch's results); lse is NaN, or -inf for a row of
 *                                -inf.  Other rows are untouched.
 *
 * fewbit_hipx_cross_entropy_host: HOST pointers, no device is touched.  logits_host rows x width fp32, contiguous (pass the values of a 16-bit
 *   tensor widened); grow_host one double per row, or NULL: 1; lse_host, loss_host rows doubles; dlogits_host rows x width doubles, or NULL:
 *   no gradient.  Refuses what the launches refuse of rows, width and null pointers.
 * fewbit_hipx_cross_entropy_forward: ONE launch on `stream`; every row is read once, by one workgroup of 256 lanes; rows are taken by the
 *   width of the grid, at most 2048 workgroups.  lse, loss: rows floats each.
 * fewbit_hipx_cross_entropy_backward: ONE launch on `stream`, the same plan; every element is read once and written once.
 *   lse          what the forward wrote for these logits
 *   grow         the gradient arriving at the row's loss, a DEVICE pointer either way, so nothing is read back and both launches can be
 *                recorded into a hipGraph: grow_stride = 1: one float per row; grow_stride = 0: ONE float for every row (the gradient of a sum,
 *                or of a mean with 1 / count multiplied in)
 *   dlogits      rows x width of `dtype`, row stride ld_out >= width.  dlogits == logits with ld_out == ld is the backward IN PLACE: the
 *                gradient replaces the logits, bit for bit what the out-of-place call writes.  Any other overlap of the two is refused.
 *                The gap of a row stride is neither read nor written.
 * No alignment is asked of logits, dlogits, ld or ld_out beyond that of the element: a row is walked as [head | aligned 16-byte pieces | tail]
 * wherever it starts (a 50265-wide bf16 row starts on a 2-byte boundary); nothing outside [row, row + width) is touched.  Backward stores by
 * 16-byte pieces where the output row starts at the same offset from a 16-byte boundary as the input row, and element by element otherwise:
 * the same bytes either way.
 * Refused before anything is launched: an unknown dtype, a null pointer, grow_stride > 1, an overlap (FEWBIT_ERR_INVALID_ARGUMENT); rows outside
 * 1 .. 2^31, width outside 1 .. 2^24, ld or ld_out below the width or beyond 2^31 (FEWBIT_ERR_UNSUPPORTED).
 * Not done: a row split over several workgroups (few rows of a huge width), a wave per row for narrow rows, class weights, label smoothing
 * and probability targets, the loss fused into the GEMM of the LM head. */
int fewbit_hipx_cross_entropy_host(const float *logits_host, const int64_t *target_host, size_t rows, size_t width, int64_t ignore_index,
                                   const double *grow_host, double *lse_host, double *loss_host, double *dlogits_host);
int fewbit_hipx_cross_entropy_forward(int dtype, const void *logits, size_t rows, size_t width, size_t ld, const int64_t *target, int64_t ignore_index,
                                      float *lse, float *loss, void *stream);
int fewbit_hipx_cross_entropy_backward(int dtype, const void *logits, size_t rows, size_t width, size_t ld, const int64_t *target, int64_t ignore_index,
                                       const float *lse, const float *grow, size_t grow_stride, void *dlogits, size_t ld_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FEWBIT_HIPX_H_ */
