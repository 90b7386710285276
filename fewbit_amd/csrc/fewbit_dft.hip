// fewbit_dft.hip -- the sampled Fourier transform of the randomized linear layers (the reference's 'dft' estimator) on gfx950, the
// kernels of the companion library libfewbit_hipx.so (include/fewbit_hipx.h):
//
//     out[0][j][c] + i out[1][j][c] = scale * (1 / sqrt(N)) * sum_n M[n][c] e^{-2 pi i n idx[j] / N}     M: rows x features (bf16 / fp16 / fp32)
//
// = torch.fft.fft(M, dim=0, norm='ortho')[idx] * scale, as two planes (real, imaginary) of proj x features.  What it replaces: the
// layer's torch.fft formulation, which materialises the whole complex rows x features transform (for a 16-bit input after a cast to fp32)
// and gathers the sampled rows afterwards -- 209 / 846 us for 16384 x 768 / 3072 bf16 at p = 3276 (profiles/r06_sketch_bench.json).
//
// The machine is the sampled DCT's (fewbit_dct.hip; shared code: fewbit_fft4.h): features (2c, 2c + 1) of a row are one complex number,
// Z = DFT_N of that column is a four-step FFT (pass A along n1 with the twiddle W_N^{n2 k1}, pass B along n2), and the pass-B workgroup of
// the residue pair (u, N1 - u) holds Z[k] and Z[N - k] of every sampled k of its two classes.  Two differences:
//   pass A   loads row n = N2 n1 + b itself (no Makhoul reordering);
//   pass B   splits the packed pair, X_2c[k] = (Z[k] + conj Z[N-k]) / 2 and X_2c+1[k] = (Z[k] - conj Z[N-k]) / 2i, and writes both parts
//            times scale / sqrt(N) (no e^{-i pi k / 2N} twiddle, so no W_4N tables; no sqrt(2) at k = 0).
// Exact by construction: at k = 0 and k = N / 2 the pair is one LDS entry read twice (imaginary parts 0), and a sampled pair k, N - k
// reads the same two entries swapped (exact conjugates).  Same row counts, tiles, rows of a seed and workspace as the DCT.
// The pair contract (the DCT's): the rounding error of column c scales with the RMS of the pair (c, c ^ 1), and a NaN or Inf in one
// column makes its partner non-finite too; other columns, the padding behind ld and the memory around out are untouched.  torch.fft
// (the reference, the layer's fallback) keeps every column apart (tests/test_gpu_transform_columns.py).
// Traffic: M once + 2 x rows x features x 4 B of intermediate + 2 planes of p rows.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "fewbit_fft4.h"
#include "fewbit_hipx.h"

namespace fewbit_hip {
namespace dft {

using namespace dct;

// (fail, which every unit of the companion library reports through, is declared by fewbit_unit.h and defined below)
// (both passes: fewbit_fft4.h -- pass_a_kernel / pass_a_zext_kernel on the rows in their order, pass_b_kernel with the epilogue FourierPlanes)

// ---- host side (fewbit_fft4.h: the checks, the dispatch and the LDS opt-in of both pairs) ------------------------------------------
struct Dft {
    static constexpr const char *kName = "sampled_dft", *kWorkspace = "fewbit_hipx_sampled_dft_workspace";
    static constexpr int (*fail)(int, const char *, ...) = dft::fail;
    static constexpr bool kSeededLast = false, kZext = false;
    using Order = RowsInOrder;
    using Epilogue = FourierPlanes;
    using PassB = Dft;
};

// The zero-extended pair (fewbit_hipx_sampled_dft_zext): fewbit_fft4.h's pass_a_zext_kernel on the rows in their order, and Dft's pass B
struct DftZext {
    static constexpr const char *kName = "sampled_dft_zext", *kWorkspace = "fewbit_hipx_sampled_dft_workspace";
    static constexpr int (*fail)(int, const char *, ...) = dft::fail;
    static constexpr bool kSeededLast = false, kZext = true;
    using Order = RowsInOrder;
    using Epilogue = FourierPlanes;
    using PassB = Dft;
};

#ifndef FEWBIT_DFT_TU
#define FEWBIT_DFT_TU -1
#endif
#if FEWBIT_DFT_TU <= 0
thread_local char g_last_error[256] = "";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof g_last_error, fmt, ap);
    va_end(ap);
    return code;
}
#endif  // FEWBIT_DFT_TU <= 0

}  // namespace dft

// Three translation units, one per dtype (-DFEWBIT_DFT_TU=0 / 1 / 2 = FEWBIT_F32 / F16 / BF16): pass A reading that dtype, pass B writing
// it and its opt-in; the C entry points with unit 0.  Units 3 / 4 / 5: pass A of the zero-extended pair reading F32 / F16 / BF16 and its
// opt-in (pass B is the plain pair's, of units 0 .. 2).  Without the define everything is one unit.
#if FEWBIT_DFT_TU >= 0 && FEWBIT_DFT_TU < 3
FB_FFT4_UNIT(, dft::Dft, FEWBIT_DFT_TU)
#endif
#if FEWBIT_DFT_TU == 0
FB_FFT4_UNIT(extern, dft::Dft, FEWBIT_F16)
FB_FFT4_UNIT(extern, dft::Dft, FEWBIT_BF16)
FB_FFT4_UNIT_A(extern, dft::DftZext, FEWBIT_F32)
FB_FFT4_UNIT_A(extern, dft::DftZext, FEWBIT_F16)
FB_FFT4_UNIT_A(extern, dft::DftZext, FEWBIT_BF16)
#endif
#if FEWBIT_DFT_TU >= 3
extern template int dct::opt_in_dtype<dft::Dft, FEWBIT_DFT_TU - 3>();
FB_FFT4_UNIT_A(, dft::DftZext, FEWBIT_DFT_TU - 3)
#endif
#if FEWBIT_DFT_TU < 0
FB_FFT4_UNIT_A(, dft::DftZext, FEWBIT_F32)
FB_FFT4_UNIT_A(, dft::DftZext, FEWBIT_F16)
FB_FFT4_UNIT_A(, dft::DftZext, FEWBIT_BF16)
#endif

}  // namespace fewbit_hip

#if FEWBIT_DFT_TU <= 0
using namespace fewbit_hip;
using namespace fewbit_hip::dft;

extern "C" {

int fewbit_hipx_abi_version(void) { return FEWBIT_HIPX_ABI_VERSION; }

const char *fewbit_hipx_last_error(void) { return g_last_error; }

size_t fewbit_hipx_sampled_dft_workspace(int dtype, size_t rows, size_t features, size_t proj) {
    Split sp;
    if (!known_dtype(dtype) || features == 0 || proj == 0 || !split_rows(rows, sp)) return 0;
    return workspace_bytes_of(rows, features, proj);
}

int fewbit_hipx_sampled_dft(int dtype, const void *m, size_t rows, size_t features, size_t ld, const int64_t *idx, size_t proj, double scale, int out_dtype,
                            void *out, void *workspace, size_t workspace_bytes, void *stream) {
    return run<Dft>(dtype, out_dtype, m, rows, rows, features, ld, RowsInMemory{idx}, proj, scale, out, workspace, workspace_bytes, stream);
}

int fewbit_hipx_sampled_dft_seeded(int dtype, const void *m, size_t rows, size_t features, size_t ld, uint64_t seed, const uint64_t *seed_device, size_t proj,
                                   double scale, int out_dtype, void *out, void *workspace, size_t workspace_bytes, void *stream) {
    return run<Dft>(dtype, out_dtype, m, rows, rows, features, ld, rows_of_seed(seed, seed_device), proj, scale, out, workspace, workspace_bytes, stream);
}

size_t fewbit_hipx_sampled_rows_ceil(size_t rows) { return rows_ceil(rows); }

int fewbit_hipx_sampled_dft_zext(int dtype, const void *m, size_t rows, size_t valid_rows, size_t features, size_t ld, const int64_t *idx, size_t proj,
                                 double scale, int out_dtype, void *out, void *workspace, size_t workspace_bytes, void *stream) {
    return run<DftZext>(dtype, out_dtype, m, rows, valid_rows, features, ld, RowsInMemory{idx}, proj, scale, out, workspace, workspace_bytes, stream);
}

int fewbit_hipx_sampled_dft_zext_seeded(int dtype, const void *m, size_t rows, size_t valid_rows, size_t features, size_t ld, uint64_t seed,
                                        const uint64_t *seed_device, size_t proj, double scale, int out_dtype, void *out, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    return run<DftZext>(dtype, out_dtype, m, rows, valid_rows, features, ld, rows_of_seed(seed, seed_device), proj, scale, out, workspace, workspace_bytes, stream);
}

}  // extern "C"
#endif  // FEWBIT_DFT_TU <= 0
