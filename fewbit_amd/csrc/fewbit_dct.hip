// fewbit_dct.hip -- the sampled cosine transform of the randomized linear layers (the reference's 'dct' estimator)
// on gfx950:
//
//     out[j][:] = scale * DCT-II_ortho(M, along the rows)[idx[j]][:]        M: rows x features (bf16 / fp16 / fp32), rows = 2^m or 3, 5, 7, 9, 15 x 2^m
//
// What it replaces in the reference (skolai/fewbit): `dct(input_view, dim=0, norm='ortho')[proj, ...]` in LinearGRPFunc.forward
// (fewbit/functional/linear.py:113-122) and the same on the gradient in .backward (:174-183); dct = fewbit/fft.py:10-43 (shuffle,
// torch.fft.fft along the transposed last dimension, phase multiply).  There the WHOLE transform is materialised in fp32 (for a
// 16-bit input after a cast) through a strided library FFT and the sampled rows are gathered afterwards: measured here 443 us /
// 1679 us for 16384 x 768 / 3072 bf16 (profiles/r06_sketch_bench.json), 110-120 x the bytes the result needs (read M once, write
// p rows).  This kernel pair moves M once, one fp32 intermediate once out and once back, and writes only the sampled rows.
//
// ---- the algorithm ---------------------------------------------------------------------------------------------------------
//   1. Makhoul's reordering (the reference's step 1, fewbit/fft.py:26): v[n] = x[2n] (n < N/2), v[N-1-n] = x[2n+1]; with
//      V = DFT_N(v):  DCT-II(x)[k] = Re(2 e^{-i pi k / 2N} V[k]).
//   2. Two real columns per complex transform: M is row-major, so features (2c, 2c+1) of a row ARE a complex number in memory;
//      Z = DFT_N(v_2c + i v_2c+1) gives V_2c[k] = (Z[k] + conj Z[N-k]) / 2 and V_2c+1[k] = (Z[k] - conj Z[N-k]) / 2i.
//      The pair contract: the rounding error of column c scales with the RMS of the pair (c, c ^ 1), not with its own, and a NaN or Inf
//      in one column makes its partner non-finite too; other columns, the padding behind ld and the memory around out are untouched.
//      torch.fft (the reference, the layer's fallback) keeps every column apart (tests/test_gpu_transform_columns.py).
//   3. Four-step DFT, N = N1 x N2 (each 16 .. 512; 16384 = 128 x 128, 262144 = 512 x 512; 12288 = 128 x 96: the odd factor 3, 5, 7, 9 or 15 goes to N2), n = N2 n1 + n2, k = k1 + N1 k2:
//          pass A   for every n2:  A[k1][n2] = W_N^{n2 k1} * sum_{n1} z[N2 n1 + n2] W_N1^{n1 k1}        (length-N1 DFTs over rows N2 apart)
//          pass B   for every k1:  Z[k1 + N1 k2] = sum_{n2} A[k1][n2] W_N2^{n2 k2}                       (length-N2 DFTs, contiguous)
//      Pass B never writes Z: the workgroup that owns the residues k1 and N1 - k1 holds Z[k] AND Z[N-k] for every k of those
//      two classes in LDS, reads the samples of those classes (sorted by class in pass A) and writes just those rows of the result.
//
// ---- tiling ------------------------------------------------------------------------------------------------------------------
//   tile        L points x 32 complex fp32 entries = 32 KiB of LDS at L = 128 (+ 3-7 KiB of tables): FOUR 256-thread workgroups per CU
//               (L = 256, from 32768 rows on: 64 KiB, two per CU).
//               Lanes run along the 32 entries of a point: every LDS access of a half-wave is 256 contiguous bytes (all 64 banks once,
//               ds_read/write_b64: conflict-free), every twiddle is half-wave-uniform (an LDS broadcast).
//   FFT         in place, decimation in frequency, TWO stages at L = 128 (radix 16 then radix 8, each butterfly entirely in the
//               registers of one thread; 64 = 8 x 8, 32 = 8 x 4, 16 = 16; 96 = 3 x 8 x 4, 192 = 3 x 8 x 8, 48 = 3 x 16, 112 = 7 x 16, 144 = 3 x 3 x 16, 240 = 3 x 5 x 16), one barrier per stage; the result stands in digit-reversed
//               positions (pos_to_freq / freq_to_pos), which costs nothing: both passes address their outputs through the map.
//   pass A      workgroup (b, t): the rows n = N2 n1 + b of column tile t (32 complex columns = 64 features).  Loads N1 row segments
//               (128 B of bf16: full cache lines, 16 B per lane, issued back to back), converts to fp32, transforms along n1,
//               multiplies by W_N^{n2 k1} (two table lookups, one complex multiply) and writes the intermediate per HALF tile,
//               [half tile][k1][n2][16 columns]: 128 contiguous bytes per (k1, half).
//   pass B      workgroup (u, t): residues k1 = u and N1 - u of half tile t (16 complex columns).  Its 32 entries per point are the two
//               residue rows side by side, so one butterfly serves both.  Reads two contiguous N2 x 128 B blocks, transforms along n2 and
//               writes the samples of its two residue classes: four lanes per sampled row (four complex columns each), 64 rows at a time,
//               e^{-i pi k / 2N} from two small tables (no transcendental per sample).
//   idx         an int64 array of the caller (fewbit_hip_sampled_dct, RowsInMemory) or a FUNCTION of a 64-bit seed (fewbit_hip_sampled_dct_seeded,
//               RowsOfSeed: Philox4x32-10) -- what the layer uses: no array, no launch that draws one, a seed to keep for backward, capturable
//               into a hipGraph.  Either way ONE workgroup of pass A sorts the samples by residue class into the workspace (sort_rows), so
//               that a pass-B workgroup reads exactly its own (each of them testing all of idx was a third of pass B's time).
//   traffic     M once + 2 x rows x features x 4 B of intermediate + the p sampled rows: 16384 x 768 bf16, p = 3276: 25 + 2 x 50 + 5 MB.
// Measured and not kept (round 6, profiles/r06_dct_variants.txt): 64 KiB tiles with 512-thread workgroups (same time); persistent
// workgroups that request the next tile before transforming the current one (the radix-16 butterfly leaves no registers for it: spills).
// Roofline class: HBM / Infinity Cache bandwidth (5 N log2 N flops per column: 0.9 GFLOP for 16384 x 768).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "fewbit_core.h"       // (fail: shared with the core unit of fewbit_kernels.hip)
#include "fewbit_fft4.h"
#include "fewbit_hip.h"
#include "fewbit_philox.h"

// Units 0 .. 2 (and the single-unit build) are libfewbit_hip.so's.  Units 3 .. 5 (-DFEWBIT_DCT_TU=3 / 4 / 5 = FEWBIT_F32 / F16 / BF16 + 3) are
// the companion library's: the zero-extended DCT (fewbit_hipx_sampled_dct_zext, include/fewbit_hipx.h) -- pass A is fewbit_fft4.h's
// pass_a_zext_kernel in Makhoul's order, pass B is the DCT's, compiled a second time under a name of its own (CosineRows<CompanionLibrary>).
#ifndef FEWBIT_DCT_TU
#define FEWBIT_DCT_TU -1
#endif
#if FEWBIT_DCT_TU >= 3
#include "fewbit_hipx.h"
#endif

namespace fewbit_hip {
namespace dct {

// (tiles, small transforms, row loads, tables, the rows of a seed and their sort, both passes -- pass_a_kernel / pass_a_zext_kernel in
// Makhoul's order, pass_b_kernel with the epilogue CosineRows --, split_rows, the host side: fewbit_fft4.h)

// ---- host side (fewbit_fft4.h: the checks, the dispatch and the LDS opt-in of both pairs) ------------------------------------------
#if FEWBIT_DCT_TU < 3
struct Dct {
    static constexpr const char *kName = "sampled_dct", *kWorkspace = "fewbit_hip_sampled_dct_workspace";
    static constexpr int (*fail)(int, const char *, ...) = fewbit_hip::fail;
    static constexpr bool kSeededLast = true, kZext = false;
    using Order = RowsMakhoul;
    using Epilogue = CosineRows<CoreLibrary>;
    using PassB = Dct;
};

// The file is compiled as three translation units in parallel, one per dtype (-DFEWBIT_DCT_TU=0 / 1 / 2 = FEWBIT_F32 / F16 / BF16: 114
// kernels each; the C entry points with unit 0), and linked into the one library -- 50 s instead of 2.5 min; without the define everything
// is one unit (make variant).
#if FEWBIT_DCT_TU >= 0
FB_FFT4_UNIT(, Dct, FEWBIT_DCT_TU)
#endif
#if FEWBIT_DCT_TU == 0
FB_FFT4_UNIT(extern, Dct, FEWBIT_F16)
FB_FFT4_UNIT(extern, Dct, FEWBIT_BF16)
#endif
#else  // FEWBIT_DCT_TU >= 3: the zero-extended pair of the companion library (its error text: fewbit_hipx_last_error)
}  // namespace dct
namespace dft {
FEWBIT_HIDDEN int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
}
namespace dct {
struct DctZext {
    static constexpr const char *kName = "sampled_dct_zext", *kWorkspace = "fewbit_hipx_sampled_dft_workspace";
    static constexpr int (*fail)(int, const char *, ...) = dft::fail;
    static constexpr bool kSeededLast = false, kZext = true;
    using Order = RowsMakhoul;
    using Epilogue = CosineRows<CompanionLibrary>;
    using PassB = DctZext;
};

// three units, one per dtype: 76 pass A and 38 pass B kernels each; the C entry points with unit 3
FB_FFT4_UNIT(, DctZext, FEWBIT_DCT_TU - 3)
#if FEWBIT_DCT_TU == 3
FB_FFT4_UNIT(extern, DctZext, FEWBIT_F16)
FB_FFT4_UNIT(extern, DctZext, FEWBIT_BF16)
#endif
#endif  // FEWBIT_DCT_TU < 3

}  // namespace dct
}  // namespace fewbit_hip

#if FEWBIT_DCT_TU <= 0
using namespace fewbit_hip;
using namespace fewbit_hip::dct;

extern "C" {

size_t fewbit_hip_sampled_dct_workspace(int dtype, size_t rows, size_t features, size_t proj) {
    Split sp;
    (void)dtype;
    if (features == 0 || proj == 0 || !split_rows(rows, sp)) return 0;
    return workspace_bytes_of(rows, features, proj);
}

int fewbit_hip_sampled_dct(int dtype, const void *m, size_t rows, size_t features, size_t ld, const int64_t *idx, size_t proj, double scale, void *out,
                           void *workspace, size_t workspace_bytes, void *stream) {
    return run<Dct>(dtype, dtype, m, rows, rows, features, ld, RowsInMemory{idx}, proj, scale, out, workspace, workspace_bytes, stream);
}

int fewbit_hip_sampled_dct_seeded(int dtype, const void *m, size_t rows, size_t features, size_t ld, uint64_t seed, const uint64_t *seed_device, size_t proj,
                                  double scale, void *out, void *workspace, size_t workspace_bytes, void *stream) {
    return run<Dct>(dtype, dtype, m, rows, rows, features, ld, rows_of_seed(seed, seed_device), proj, scale, out, workspace, workspace_bytes, stream);
}

int fewbit_hip_sampled_rows(uint64_t seed, size_t rows, size_t proj, int64_t *idx) {
    Split sp;
    if (!split_rows(rows, sp)) return refuse_rows<Dct>("sampled_rows", rows);
    if (proj > 0 && idx == nullptr) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "sampled_rows: null pointer");
    const sketch::Key key = sketch::key_of(seed);
    const bool pow2 = draws_halves(rows);
    const size_t per = per_draw(pow2);
    for (size_t q = 0; per * q < proj; ++q) {
        uint32_t w[4];
        sketch::philox4x32(static_cast<uint32_t>(q), static_cast<uint32_t>(q >> 32), 0u, kRowsDomain, key, w);
        for (size_t h = 0; h < per && per * q + h < proj; ++h)
            idx[per * q + h] = pow2 ? static_cast<int64_t>(drawn_row<true>(w, static_cast<int>(h), 0u) & (rows - 1))
                                    : static_cast<int64_t>(drawn_row<false>(w, static_cast<int>(h), static_cast<uint32_t>(rows)));
    }
    return FEWBIT_OK;
}

}  // extern "C"
#endif  // FEWBIT_DCT_TU <= 0

#if FEWBIT_DCT_TU == 3
using namespace fewbit_hip;
using namespace fewbit_hip::dct;

extern "C" {

int fewbit_hipx_sampled_dct_zext(int dtype, const void *m, size_t rows, size_t valid_rows, size_t features, size_t ld, const int64_t *idx, size_t proj,
                                 double scale, void *out, void *workspace, size_t workspace_bytes, void *stream) {
    return run<DctZext>(dtype, dtype, m, rows, valid_rows, features, ld, RowsInMemory{idx}, proj, scale, out, workspace, workspace_bytes, stream);
}

int fewbit_hipx_sampled_dct_zext_seeded(int dtype, const void *m, size_t rows, size_t valid_rows, size_t features, size_t ld, uint64_t seed,
                                        const uint64_t *seed_device, size_t proj, double scale, void *out, void *workspace, size_t workspace_bytes,
                                        void *stream) {
    return run<DctZext>(dtype, dtype, m, rows, valid_rows, features, ld, rows_of_seed(seed, seed_device), proj, scale, out, workspace, workspace_bytes, stream);
}

}  // extern "C"
#endif  // FEWBIT_DCT_TU == 3
