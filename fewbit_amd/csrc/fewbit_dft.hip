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

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "fewbit_fft4.h"
#include "fewbit_hipx.h"

#define FEWBIT_HIDDEN __attribute__((visibility("hidden")))

namespace fewbit_hip {
namespace dft {

using namespace dct;

FEWBIT_HIDDEN int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// ---- pass A: dct_pass_a_kernel (fewbit_dct.hip) line for line, except the row each n1 loads -------------------------------------
// (a copy, not a shared body: the DCT's kernels stay bit for bit the machine code they were measured as; routing them through a
// common inline function changed the instruction schedule of 44 of them)
// grid (N2, column tiles): workgroup (b, t) transforms the rows n = N2 n1 + b of column tile t (of M itself).  inter: [half tile][k1][n2][16] complex fp32.
template <int DT, int N1, int N2, typename ROWS>
__global__ __launch_bounds__(kThreadsA, (N1 > 128 ? 2 : 4)) void dft_pass_a_kernel(const void *__restrict__ x, size_t features, size_t ld, f32x2 *__restrict__ inter, ROWS rows,
                                                                  size_t proj, int *__restrict__ offsets, Sample *__restrict__ sorted) {
    constexpr int N = N1 * N2, kCoarse = coarse_entries(N), kThreads = kThreadsA, kSlots = kThreads / C;
    static_assert(kRowsA == 1, "one n2 per workgroup");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    f32x2 *tile = reinterpret_cast<f32x2 *>(lds_raw);                 // [N1][C]
    f32x2 *tw = tile + N1 * C;                                        // W_N1^m, m < N1
    f32x2 *fine = tw + N1, *coarse = fine + kFine;                    // W_N^m (m < 128), W_N^{128 m}
    const int tid = threadIdx.x, c = tid % C, slot = tid / C;
    const int b = blockIdx.x;
    const size_t t = blockIdx.y, f0 = t * kFeatures;
    // one workgroup of the launch sorts the sampled rows for pass B first (~2 us of its own time; the launch takes 16)
    if (blockIdx.x == 0 && blockIdx.y == 0) sort_rows<N1, N, ROWS>(rows, proj, offsets, sorted, reinterpret_cast<int *>(lds_raw), tid);

    // ---- loads first (all in flight), tables while they travel, then registers -> LDS
    constexpr int PF = In<DT>::kPieceFeatures, PPS = In<DT>::kPiecesPerSegment, kTotal = N1 * PPS, kPieces = (kTotal + kThreads - 1) / kThreads;
    // (one body per case, FULL tile or edge tile, each with its own registers from the loads to the LDS writes: were the two
    // cases to meet in one set of registers in between, the copies at the join would wait for the loads right behind their issue)
    auto fill_tile = [&](auto full) __attribute__((always_inline)) {
        u32x4 raw[kPieces];
#pragma unroll
        for (int i = 0; i < kPieces; ++i) {
            const int pid = tid + kThreads * i, n1 = pid / PPS, piece = pid % PPS;
            if (kTotal % kThreads != 0 && pid >= kTotal) break;
            const size_t row = static_cast<size_t>(N2 * n1 + b);                 // (the DCT loads row 2n or 2 (N - 1 - n) + 1 here)
            raw[i] = load_piece<DT, decltype(full)::value>(x, row, ld, f0, piece, features);
        }
        for (int m = tid; m < N1; m += kThreads) tw[m] = unit(m, N1);
        for (int m = tid; m < kFine; m += kThreads) fine[m] = unit(m, N);
        for (int m = tid; m < kCoarse; m += kThreads) coarse[m] = unit(m * kFine, N);
#pragma unroll
        for (int i = 0; i < kPieces; ++i) {
            const int pid = tid + kThreads * i, n1 = pid / PPS, piece = pid % PPS;
            if (kTotal % kThreads != 0 && pid >= kTotal) break;
            float v[PF];
            unpack_piece<DT>(raw[i], v);
            f32x4 *dst = reinterpret_cast<f32x4 *>(tile + n1 * C + piece * (PF / 2));
#pragma unroll
            for (int e = 0; e < PF / 4; ++e) dst[e] = f32x4{v[4 * e], v[4 * e + 1], v[4 * e + 2], v[4 * e + 3]};
        }
    };
    if (f0 + kFeatures <= features) fill_tile(std::true_type{});       // (workgroup-uniform)
    else fill_tile(std::false_type{});
    __syncthreads();

    fft_tile<N1, kRowsA, kSlots>(tile, tw, c, slot);

    // ---- twiddle + store: unit = two complex columns (16 B) of one position P; 16 consecutive lanes = the 256 contiguous bytes of one k1
    constexpr int kUnitsTotal = N1 * (C / 2), kUnits = (kUnitsTotal + kThreads - 1) / kThreads;
#pragma unroll
    for (int i = 0; i < kUnits; ++i) {
        const int uid = tid + kThreads * i, c2 = uid % (C / 2), p = uid / (C / 2);
        if (kUnitsTotal % kThreads != 0 && uid >= kUnitsTotal) break;
        const int k1 = pos_to_freq<N1>(p), e = b * k1;
        const f32x2 w = table_unit(fine, coarse, e, kCoarse > 1);
        const f32x4 z = *reinterpret_cast<const f32x4 *>(tile + p * C + 2 * c2);
        const f32x2 a = cmul(f32x2{z[0], z[1]}, w), bb = cmul(f32x2{z[2], z[3]}, w);
        // (the intermediate is kept per HALF tile of 16 complex columns -- what one pass-B workgroup reads: 128 contiguous bytes here)
        f32x4 *dst = reinterpret_cast<f32x4 *>(inter + (((2 * t + c2 / (CB / 2)) * N1 + k1) * N2 + b) * CB + 2 * (c2 % (CB / 2)));
        *dst = f32x4{a.x, a.y, bb.x, bb.y};
    }
}

// ---- pass B: the DCT's, with the Fourier epilogue -----------------------------------------------------------------------------
// grid (N1 / 2 + 1, half tiles of 16 complex columns): residues k1 = u and (N1 - u) % N1; LDS tile [N2][2][16] (fewbit_dct.hip).
// out: [2][proj][features] in ODT (real plane, imaginary plane); factor = scale / sqrt(N).
template <int ODT, int N1, int N2>
__global__ __launch_bounds__(kThreadsB, (N2 > 128 ? 2 : 4)) void dft_pass_b_kernel(const f32x2 *__restrict__ inter, const int *__restrict__ offsets, const Sample *__restrict__ sorted,
                                                                  size_t proj, size_t features, float factor, void *__restrict__ out) {
    constexpr int kThreads = kThreadsB, kSlots = kThreads / C;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    f32x2 *tile = reinterpret_cast<f32x2 *>(lds_raw);                 // [N2][2][CB]
    f32x2 *tw = tile + N2 * 2 * CB;                                   // W_N2^m
    const int tid = threadIdx.x;
    const int u = blockIdx.x, k1a = u, k1b = (N1 - u) % N1;
    const size_t t = blockIdx.y, f0 = t * (2 * CB);
    constexpr int kLanes = kServeLanes, E = CB / kLanes, kSGroups = kThreads / kLanes;       // lanes per sample, complex columns per lane
    const int lane = tid % kLanes, sgroup = tid / kLanes;

    // this workgroup's samples first (vmcnt counts in order), unconditionally (a clamped index), as in the DCT
    const int begin = offsets[u], count = offsets[u + 1] - begin;
    constexpr int kPre = 2;
    Sample pre[kPre];
#pragma unroll
    for (int i = 0; i < kPre; ++i) {
        const size_t e = static_cast<size_t>(begin) + sgroup + i * kSGroups;
        pre[i] = sorted[e < proj ? e : proj - 1];
    }
    constexpr int kPerRow = N2 * (CB / 2), kTotal = 2 * kPerRow, kPieces = (kTotal + kThreads - 1) / kThreads;     // 16-byte pieces (two complex)
    f32x4 v[kPieces];
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
        const int pid = tid + kThreads * i, r = pid / kPerRow, rest = pid % kPerRow;
        if (kTotal % kThreads != 0 && pid >= kTotal) break;
        const f32x2 *src = inter + (t * N1 + (r == 0 ? k1a : k1b)) * static_cast<size_t>(N2) * CB;
        v[i] = reinterpret_cast<const f32x4 *>(src)[rest];
    }
    for (int m = tid; m < N2; m += kThreads) tw[m] = unit(m, N2);
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
        const int pid = tid + kThreads * i, r = pid / kPerRow, rest = pid % kPerRow, n2 = rest / (CB / 2), c2 = rest % (CB / 2);
        if (kTotal % kThreads != 0 && pid >= kTotal) break;
        *reinterpret_cast<f32x4 *>(tile + (n2 * 2 + r) * CB + 2 * c2) = v[i];
    }
    __syncthreads();
    fft_tile<N2, 1, kSlots>(tile, tw, tid % C, tid / C);               // (ends with a barrier)

    const float half = 0.5f * factor;
    const size_t plane = proj * features;
    auto write_row = [&](int km, size_t j) __attribute__((always_inline)) {
        const int k1 = km % N1, k2 = km / N1;
        const int r = k1 == k1a ? 0 : 1;
        const int k2m = k1 == 0 ? (N2 - k2) % N2 : N2 - 1 - k2;         // N - k = (N1 - k1) + N1 k2m
        const f32x2 *pk = tile + (freq_to_pos<N2>(k2) * 2 + r) * CB + E * lane;
        const f32x2 *pm = tile + (freq_to_pos<N2>(k2m) * 2 + (1 - r)) * CB + E * lane;
        f32x2 zk[E], zm[E];
        if constexpr (E >= 2) {
#pragma unroll
            for (int e = 0; e < E; e += 2) {
                const f32x4 a4 = *reinterpret_cast<const f32x4 *>(pk + e), b4 = *reinterpret_cast<const f32x4 *>(pm + e);
                zk[e] = f32x2{a4[0], a4[1]}; zk[e + 1] = f32x2{a4[2], a4[3]};
                zm[e] = f32x2{b4[0], b4[1]}; zm[e + 1] = f32x2{b4[2], b4[3]};
            }
        } else {
            zk[0] = pk[0]; zm[0] = pm[0];
        }
        // a = Z[k], b = Z[N - k]:  X_2c = (a + conj b) / 2,  X_2c+1 = (a - conj b) / 2i = ((a.y + b.y) + i (b.x - a.x)) / 2
        float re[2 * E], im[2 * E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const f32x2 a = zk[e], b = zm[e];
            re[2 * e] = (a.x + b.x) * half;
            im[2 * e] = (a.y - b.y) * half;
            re[2 * e + 1] = (a.y + b.y) * half;
            im[2 * e + 1] = (b.x - a.x) * half;
        }
        const size_t fa = f0 + 2 * E * lane, at = j * features + fa;
        store_values<ODT, E>(out, at, re, fa, features);
        store_values<ODT, E>(out, plane + at, im, fa, features);
    };
#pragma unroll
    for (int i = 0; i < kPre; ++i)
        if (sgroup + i * kSGroups < count) write_row(pre[i].k, static_cast<size_t>(pre[i].j));
    for (int e = sgroup + kPre * kSGroups; e < count; e += kSGroups) {
        const Sample smp = sorted[static_cast<size_t>(begin) + e];
        write_row(smp.k, static_cast<size_t>(smp.j));
    }
}

// ---- host side (fewbit_fft4.h: the checks, the dispatch and the LDS opt-in of both pairs) ------------------------------------------
struct Dft {
    static constexpr const char *kName = "sampled_dft", *kWorkspace = "fewbit_hipx_sampled_dft_workspace";
    static constexpr int (*fail)(int, const char *, ...) = dft::fail;
    static constexpr bool kSeededLast = false, kZext = false;
    using PassB = Dft;
    template <int DT> static int opt_in_b() { return opt_in_dtype<Dft, DT>(); }                // (of both passes: the pair has one opt-in)
    template <int DT, int N1, int N2, typename ROWS> static constexpr auto pass_a() { return &dft_pass_a_kernel<DT, N1, N2, ROWS>; }
    template <int ODT, int N1, int N2> static constexpr auto pass_b() { return &dft_pass_b_kernel<ODT, N1, N2>; }
    template <int N1, int N2> static constexpr size_t lds_b() { return (2 * N2 * CB + N2) * sizeof(f32x2); }      // (no W_4N tables)
    static float factor(double scale, size_t rows) { return static_cast<float>(scale / std::sqrt(static_cast<double>(rows))); }
};

// The zero-extended pair (fewbit_hipx_sampled_dft_zext): fewbit_fft4.h's pass_a_zext_kernel on the rows in their order, and Dft's pass B
struct DftZext {
    static constexpr const char *kName = "sampled_dft_zext", *kWorkspace = "fewbit_hipx_sampled_dft_workspace";
    static constexpr int (*fail)(int, const char *, ...) = dft::fail;
    static constexpr bool kSeededLast = false, kZext = true;
    using PassB = Dft;
    template <int DT, int N1, int N2, typename ROWS> static constexpr auto pass_a() { return &pass_a_zext_kernel<RowsInOrder, DT, N1, N2, ROWS>; }
    static float factor(double scale, size_t rows) { return Dft::factor(scale, rows); }
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
