// fewbit_signed.hip -- the sampled DCT and DFT with a random sign per input row (companion library, include/fewbit_hipx.h):
//
//     out = scale * T(D m)[rows(seed)]        T: the orthonormal DCT-II or the DFT of length `rows`, D = diag(+-1) of the same seed
//
// S = sqrt(N / p) R T D is the subsampled randomized transform the variance analysis of the estimator assumes: E[S^T S] = D T^H T D = I for
// every D, and D flattens the row energies of T D m -- without it whatever many rows of m share (a mean activation, a repeated token) lands
// in a few rows of T m, which p samples hit or miss.  The signs are a function of (seed, row) that host and kernel evaluate alike
// (fewbit_fft4.h: row_flipped); nothing is kept for backward but the seed the sampled rows already need.
// Kernels: pass A is fewbit_fft4.h's pass_a_zext_kernel with ROWS = SignedRowsOfSeed (the raw 16-byte pieces are XORed with their sign bits
// before they are unpacked); pass B, the workspace and the intermediate are the zero-extended pairs' (fewbit_dct.hip units 3 .. 5,
// fewbit_dft.hip).  Three translation units, one per dtype (-DFEWBIT_SIGNED_TU=0 / 1 / 2 = FEWBIT_F32 / F16 / BF16: 76 pass A kernels
// each, both row orders; the C entry points with unit 0); without the define everything is one unit.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "fewbit_fft4.h"
#include "fewbit_hipx.h"

#ifndef FEWBIT_SIGNED_TU
#define FEWBIT_SIGNED_TU -1
#endif

namespace fewbit_hip {
namespace dct {
struct DctZext;                             // (fewbit_dct.hip, units 3 .. 5: its opt-in and its pass B are linked, not compiled again)
}
namespace dft {
using namespace dct;
struct Dft;                                 // (fewbit_dft.hip)
struct DftZext;                             // (fail: fewbit_unit.h)
}

#define FB_SIGNED_LINKED(DT)                                                                                                   \
    extern template int dct::opt_in_dtype<dct::DctZext, DT>();                                                                 \
    extern template int dct::opt_in_dtype<dft::DftZext, DT>();                                                                 \
    FB_FFT4_UNIT_B(extern, dct::DctZext, DT)                                                                                   \
    FB_FFT4_UNIT_B(extern, dft::Dft, DT)
FB_SIGNED_LINKED(FEWBIT_F32)
FB_SIGNED_LINKED(FEWBIT_F16)
FB_SIGNED_LINKED(FEWBIT_BF16)
#undef FB_SIGNED_LINKED

namespace dft {

struct DctSigned {
    static constexpr const char *kName = "sampled_dct_signed", *kWorkspace = "fewbit_hipx_sampled_dft_workspace";
    static constexpr int (*fail)(int, const char *, ...) = dft::fail;
    static constexpr bool kSeededLast = false, kZext = true;
    using Order = RowsMakhoul;
    using Epilogue = CosineRows<CompanionLibrary>;
    using PassB = DctZext;
    using Unsigned = DctZext;
};

struct DftSigned {
    static constexpr const char *kName = "sampled_dft_signed", *kWorkspace = "fewbit_hipx_sampled_dft_workspace";
    static constexpr int (*fail)(int, const char *, ...) = dft::fail;
    static constexpr bool kSeededLast = false, kZext = true;
    using Order = RowsInOrder;
    using Epilogue = FourierPlanes;
    using PassB = Dft;
    using Unsigned = DftZext;
};

}  // namespace dft

#if FEWBIT_SIGNED_TU >= 0
FB_FFT4_UNIT_SIGNED(, dft::DctSigned, FEWBIT_SIGNED_TU)
FB_FFT4_UNIT_SIGNED(, dft::DftSigned, FEWBIT_SIGNED_TU)
#endif
#if FEWBIT_SIGNED_TU == 0
FB_FFT4_UNIT_SIGNED(extern, dft::DctSigned, FEWBIT_F16)
FB_FFT4_UNIT_SIGNED(extern, dft::DctSigned, FEWBIT_BF16)
FB_FFT4_UNIT_SIGNED(extern, dft::DftSigned, FEWBIT_F16)
FB_FFT4_UNIT_SIGNED(extern, dft::DftSigned, FEWBIT_BF16)
#endif

}  // namespace fewbit_hip

#if FEWBIT_SIGNED_TU <= 0
using namespace fewbit_hip;
using namespace fewbit_hip::dft;

static SignedRowsOfSeed signed_rows_of_seed(uint64_t seed, const uint64_t *device) {
    SignedRowsOfSeed rows;
    rows.value = sketch::key_of(seed);
    rows.device = reinterpret_cast<const sketch::Key *>(device);
    return rows;
}

extern "C" {

int fewbit_hipx_sampled_signs(uint64_t seed, uint64_t first, size_t count, uint8_t *flip_host) {
    if (count > 0 && flip_host == nullptr) return dft::fail(FEWBIT_ERR_INVALID_ARGUMENT, "sampled_signs: null pointer");
    const sketch::Key key = sketch::key_of(seed);
    for (size_t i = 0; i < count; ++i) flip_host[i] = row_flipped(key, first + i) ? 1 : 0;
    return FEWBIT_OK;
}

int fewbit_hipx_sampled_dct_signed(int dtype, const void *m, size_t rows, size_t valid_rows, size_t features, size_t ld, uint64_t seed,
                                   const uint64_t *seed_device, size_t proj, double scale, void *out, void *workspace, size_t workspace_bytes, void *stream) {
    return run<DctSigned>(dtype, dtype, m, rows, valid_rows, features, ld, signed_rows_of_seed(seed, seed_device), proj, scale, out, workspace, workspace_bytes, stream);
}

int fewbit_hipx_sampled_dft_signed(int dtype, const void *m, size_t rows, size_t valid_rows, size_t features, size_t ld, uint64_t seed,
                                   const uint64_t *seed_device, size_t proj, double scale, int out_dtype, void *out, void *workspace, size_t workspace_bytes,
                                   void *stream) {
    return run<DftSigned>(dtype, out_dtype, m, rows, valid_rows, features, ld, signed_rows_of_seed(seed, seed_device), proj, scale, out, workspace, workspace_bytes, stream);
}

}  // extern "C"
#endif  // FEWBIT_SIGNED_TU <= 0
