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
 * What is declared below is what a binding needs (tests/test_dft_host.py pins the exported symbol list). */
#define FEWBIT_HIPX_ABI_VERSION 1

int fewbit_hipx_abi_version(void);
const char *fewbit_hipx_last_error(void);

/* ------------------------------------------------------------------------------------------------------------------
 * Sampled Fourier transform of the randomized linear layers:
 *     out[0][j][c] + i out[1][j][c] = scale * (1 / sqrt(rows)) * sum_n m[n][c] exp(-2 pi i n idx[j] / rows)
 *   = torch.fft.fft(m, dim=0, norm='ortho')[idx] * scale, the layer's torch.fft formulation, which builds the whole complex
 *     rows x features transform before it gathers the sampled rows
 *   m    rows x features, row-major with leading dimension `ld` (elements), dtype F32 / F16 / BF16; rows = 2^k in [256, 262144],
 *        3 x 2^k in [768, 49152] or 5 x 2^k in [1280, 40960], the row counts of fewbit_hip_sampled_dct (anything else:
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

#ifdef __cplusplus
}
#endif
#endif /* FEWBIT_HIPX_H_ */
