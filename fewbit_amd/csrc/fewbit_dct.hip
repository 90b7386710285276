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

#include "fewbit_fft4.h"
#include "fewbit_hip.h"
#include "fewbit_philox.h"

// Units 0 .. 2 (and the single-unit build) are libfewbit_hip.so's.  Units 3 .. 5 (-DFEWBIT_DCT_TU=3 / 4 / 5 = FEWBIT_F32 / F16 / BF16 + 3) are
// the companion library's: the zero-extended DCT (fewbit_hipx_sampled_dct_zext, include/fewbit_hipx.h) -- pass A is fewbit_fft4.h's
// pass_a_zext_kernel in Makhoul's order, pass B is this file's, compiled a second time under a name of its own.
#ifndef FEWBIT_DCT_TU
#define FEWBIT_DCT_TU -1
#endif
#if FEWBIT_DCT_TU >= 3
#include "fewbit_hipx.h"
#endif

#define FEWBIT_HIDDEN __attribute__((visibility("hidden")))

namespace fewbit_hip {

// shared with the core unit of fewbit_kernels.hip
FEWBIT_HIDDEN int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

namespace dct {

// (tiles, small transforms, row loads, tables, the rows of a seed and their sort, split_rows, the host side: fewbit_fft4.h)

// ---- pass A -----------------------------------------------------------------------------------------------------------------
// grid (N2, column tiles): workgroup (b, t) transforms the rows n = N2 n1 + b of column tile t.  inter: [half tile][k1][n2][16] complex fp32.
template <int DT, int N1, int N2, typename ROWS>
__global__ __launch_bounds__(kThreadsA, (N1 > 128 ? 2 : 4)) void dct_pass_a_kernel(const void *__restrict__ x, size_t features, size_t ld, f32x2 *__restrict__ inter, ROWS rows,
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
            const int n = N2 * n1 + b;                                  // index into the reordered sequence v
            const size_t row = n < N / 2 ? 2 * static_cast<size_t>(n) : 2 * static_cast<size_t>(N - 1 - n) + 1;
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

// ---- pass B -----------------------------------------------------------------------------------------------------------------
#if FEWBIT_DCT_TU >= 3
inline namespace companion {                // (the companion library's copies: symbols of their own)
#endif
// grid (N1 / 2 + 1, half tiles of 16 complex columns): residues k1 = u and (N1 - u) % N1.  The LDS tile is [N2][2][16]: the two
// residue rows sit side by side, so that a half-wave still touches 256 contiguous bytes per position and one butterfly serves
// both rows -- to the transform it is one row of 32 columns.
template <int DT, int N1, int N2>
__global__ __launch_bounds__(kThreadsB, (N2 > 128 ? 2 : 4)) void dct_pass_b_kernel(const f32x2 *__restrict__ inter, const int *__restrict__ offsets, const Sample *__restrict__ sorted,
                                                                  size_t proj, size_t features, float scale, void *__restrict__ out) {
    constexpr int N = N1 * N2, kCoarse = coarse_entries(N), kThreads = kThreadsB, kSlots = kThreads / C;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    f32x2 *tile = reinterpret_cast<f32x2 *>(lds_raw);                 // [N2][2][CB]
    f32x2 *tw = tile + N2 * 2 * CB;                                   // W_N2^m
    f32x2 *fine = tw + N2, *coarse = fine + kFine;                    // W_4N^m (m < 128), W_4N^{128 m}: e^{-i pi k / 2N} = W_4N^k
    const int tid = threadIdx.x;
    const int u = blockIdx.x, k1a = u, k1b = (N1 - u) % N1;
    const size_t t = blockIdx.y, f0 = t * (2 * CB);
    // four lanes write one sampled row, four complex columns each: 64 rows at a time -- all of a typical workgroup's in one step (with 16
    // lanes per row the four dependent steps of sample -> tile -> table -> store cost 1.5 us of a 18.8 us launch, profiles/r06_dct_serve_lanes.txt)
    constexpr int kLanes = kServeLanes, E = CB / kLanes, kSGroups = kThreads / kLanes;       // lanes per sample, complex columns per lane
    const int lane = tid % kLanes, sgroup = tid / kLanes;

    // this workgroup's samples (pass A's workgroup (0, 0) sorted them): the first two of every group of lanes are requested FIRST (vmcnt
    // counts in order: looking at them after the transform does not wait for anything), unconditionally (a clamped index: hipcc gives a
    // load under a lane-divergent guard its own wait)
    const int begin = offsets[u], count = offsets[u + 1] - begin;      // (scalar loads)
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
    for (int m = tid; m < kFine; m += kThreads) fine[m] = unit(m, 4 * N);
    for (int m = tid; m < kCoarse; m += kThreads) coarse[m] = unit(m * kFine, 4 * N);
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
        const int pid = tid + kThreads * i, r = pid / kPerRow, rest = pid % kPerRow, n2 = rest / (CB / 2), c2 = rest % (CB / 2);
        if (kTotal % kThreads != 0 && pid >= kTotal) break;
        *reinterpret_cast<f32x4 *>(tile + (n2 * 2 + r) * CB + 2 * c2) = v[i];
    }
    __syncthreads();
    fft_tile<N2, 1, kSlots>(tile, tw, tid % C, tid / C);               // (ends with a barrier)

    // ---- the sampled rows of this workgroup's two residue classes: one per group of kServeLanes lanes at a time, lanes along the columns
    const float base = scale * __builtin_sqrtf(0.5f / static_cast<float>(N));          // ortho: sqrt(1 / 2N) (k > 0), sqrt(1 / 4N) (k = 0)
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
        const f32x2 w = table_unit(fine, coarse, km, kCoarse > 1);      // e^{-i pi k / 2N}
        const float f = (km == 0 ? kR2 : 1.0f) * 2.0f * base;
        float y[2 * E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            f32x2 m = zm[e];
            m.y = -m.y;                                                 // conj Z[N - k]
            const f32x2 va = (zk[e] + m) * 0.5f, d = (zk[e] - m) * 0.5f, vb = mul_mi(d);
            y[2 * e] = (w.x * va.x - w.y * va.y) * f;                   // Re(w V)
            y[2 * e + 1] = (w.x * vb.x - w.y * vb.y) * f;
        }
        const size_t fa = f0 + 2 * E * lane;
        store_values<DT, E>(out, j * features + fa, y, fa, features);
    };
#pragma unroll
    for (int i = 0; i < kPre; ++i)
        if (sgroup + i * kSGroups < count) write_row(pre[i].k, static_cast<size_t>(pre[i].j));
    // (more than 128 samples in these two classes: p beyond ~8000, or a skewed idx)
    for (int e = sgroup + kPre * kSGroups; e < count; e += kSGroups) {
        const Sample smp = sorted[static_cast<size_t>(begin) + e];
        write_row(smp.k, static_cast<size_t>(smp.j));
    }
}

#if FEWBIT_DCT_TU >= 3
}  // namespace companion
#endif

// ---- host side (fewbit_fft4.h: the checks, the dispatch and the LDS opt-in of both pairs) ------------------------------------------
#if FEWBIT_DCT_TU < 3
struct Dct {
    static constexpr const char *kName = "sampled_dct", *kWorkspace = "fewbit_hip_sampled_dct_workspace";
    static constexpr int (*fail)(int, const char *, ...) = fewbit_hip::fail;
    static constexpr bool kSeededLast = true, kZext = false;
    using PassB = Dct;
    template <int DT, int N1, int N2, typename ROWS> static constexpr auto pass_a() { return &dct_pass_a_kernel<DT, N1, N2, ROWS>; }
    template <int DT, int N1, int N2> static constexpr auto pass_b() { return &dct_pass_b_kernel<DT, N1, N2>; }
    template <int N1, int N2> static constexpr size_t lds_b() { return lds_bytes_b<N2>(N1 * N2); }
    static float factor(double scale, size_t) { return static_cast<float>(scale); }
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
    using PassB = DctZext;
    template <int DT, int N1, int N2, typename ROWS> static constexpr auto pass_a() { return &pass_a_zext_kernel<RowsMakhoul, DT, N1, N2, ROWS>; }
    template <int DT, int N1, int N2> static constexpr auto pass_b() { return &dct_pass_b_kernel<DT, N1, N2>; }
    template <int N1, int N2> static constexpr size_t lds_b() { return lds_bytes_b<N2>(N1 * N2); }
    template <int DT> static int opt_in_b() { return opt_in_pass_b<DctZext, DT>(); }
    static float factor(double scale, size_t) { return static_cast<float>(scale); }
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
