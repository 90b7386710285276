// fewbit_moments.hip -- the moments the variance estimator of the randomized linear layers needs (fewbit_amd/variance.py), on gfx950; part
// of the companion library libfewbit_hipx.so (include/fewbit_hipx.h):
//
//     row_moments   out[0] = sx  = sum_b |x_b|^2,   out[1] = sg = sum_b |g_b|^2,   out[2] = sxg = sum_b |x_b|^2 |g_b|^2
//     sum_squares   out[0] = sum_i t_i^2
//
// for X (rows x n) and G (rows x m) of independent dtypes (F32 / F16 / BF16), each element read once.  With cross = |X^T G|_F^2 (one GEMM
// and a sum_squares over its fp32 product) these four numbers give the estimator's three results.
//
// Arithmetic.  Every element is widened to fp64 (exact for all three dtypes) and folded in with ONE fp64 FMA acc = fma(v, v, acc): v * v is
// exact in fp64 (at most 24 x 2 significant bits, exponents within +-254), so the only rounding is that of the running sum.  The per-row
// sums, their product and the sums over the rows are fp64 as well: nothing overflows for finite input of any of the dtypes, and each output
// is within (terms added) * 2^-53 relative of the exact value -- exact whenever every partial sum is representable.  NaN and Inf propagate.
//
// Order.  A wave serves one row at a time: lane l adds the elements it owns in ascending order into two interleaved chains (even and odd
// positions of its pieces), the 64 lane sums go through a fixed xor butterfly (32, 16, .. 1), and the wave adds its rows in ascending order.
// A workgroup (4 waves) serves `rows per workgroup` consecutive rows, wave w the rows w, w + 4, ..; its three sums (waves added in order)
// go to the workspace.  A second launch of ONE workgroup adds the partials: wave k owns output k, lane l adds the partials l, l + 64, .. in
// ascending order, the same butterfly follows.  No floating-point atomics anywhere: the same arguments give the same bits.
//
// The plan is a pure function of the row count: rows per workgroup = max(kMinRows, ceil(rows / kMaxGroups)), workgroups = ceil(rows / rows
// per workgroup) <= kMaxGroups.  sum_squares cuts its array into pieces of kPiece elements and runs the same plan over them as rows (with
// kMinPieces in place of kMinRows).
//
// Loads.  A row is read as [head | 16-byte pieces | tail]: the head are the elements before the first 16-byte boundary (lane l loads element
// l), the pieces are aligned global_load_dwordx4, the tail the elements behind the last whole piece.  Nothing outside [row, row + n) is
// touched -- neither a row's padding nor anything beyond the last row -- whatever the leading dimension and the base pointer's offset.
//
// Cost.  Per element: the widening (one or two conversions) and one v_fma_f64, which gfx950 issues at the fp32 rate of 64 lanes per 4 cycles
// and SIMD.  16384 x (768 + 3072) bf16 is 63 M elements over 1024 SIMDs: ~3 wave instructions per 64 elements, ~12 k cycles = 5 us at
// 2.4 GHz, against ~20 us for the 126 MB at the ~6.3 TB/s a streaming read reaches: the kernel is bound by HBM, not by the fp64 VALU.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fewbit_hipx.h"
#include "fewbit_unit.h"

namespace fewbit_hip {
namespace moments {

using unit::fail, unit::known_dtype, unit::misaligned, unit::size_of;

// (tuning builds: -DFEWBIT_MOMENTS_MAX_GROUPS / _MIN_ROWS / _UNROLL; the contract, the header and the tests speak of the defaults)
#ifndef FEWBIT_MOMENTS_MAX_GROUPS
#define FEWBIT_MOMENTS_MAX_GROUPS 1024
#endif
#ifndef FEWBIT_MOMENTS_MIN_ROWS
#define FEWBIT_MOMENTS_MIN_ROWS 16
#endif
#ifndef FEWBIT_MOMENTS_UNROLL
#define FEWBIT_MOMENTS_UNROLL 2
#endif

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr size_t kMaxGroups = FEWBIT_MOMENTS_MAX_GROUPS;       // workgroups of the first launch = partials the second one adds
constexpr size_t kMinRows = FEWBIT_MOMENTS_MIN_ROWS;           // row_moments: rows per workgroup, at least (4 per wave)
constexpr size_t kPiece = 1024, kMinPieces = 4;      // sum_squares: elements per piece, pieces per workgroup at least (1 per wave)
constexpr size_t kMaxRows = size_t{1} << 31, kMaxFeatures = size_t{1} << 24;      // (rows, count and the leading dimensions; n and m)
constexpr size_t kWorkspaceBytes = kMaxGroups * 3 * sizeof(double);

struct Plan {
    size_t per_group, groups;
};
inline Plan plan(size_t rows, size_t at_least) {
    size_t per = (rows + kMaxGroups - 1) / kMaxGroups;
    per = per < at_least ? at_least : per;
    return Plan{per, (rows + per - 1) / per};
}

// (not fewbit_quantdef.h's Elem: E, the elements of a 16-byte piece, and a widening to double; fewbit_crs.hip has the same with one to float)
template <int DT> struct Elem { using type = uint16_t; static constexpr int E = 8; };
template <> struct Elem<FEWBIT_F32> { using type = uint32_t; static constexpr int E = 4; };

template <int DT> __device__ __forceinline__ double widen(typename Elem<DT>::type raw) {
    if constexpr (DT == FEWBIT_F32) return static_cast<double>(__builtin_bit_cast(float, raw));
    else if constexpr (DT == FEWBIT_BF16) return static_cast<double>(__builtin_bit_cast(float, static_cast<uint32_t>(raw) << 16));
    else return static_cast<double>(static_cast<float>(__builtin_bit_cast(_Float16, raw)));
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d /= 2) v += __shfl_xor(v, d, 64);
    return v;                                           // every lane holds the same bits (a + b == b + a)
}

// the sum of squares of the n elements at p, over the wave: lane sums in the fixed order of the header, then the butterfly
template <int DT> __device__ __forceinline__ double span_sum(const typename Elem<DT>::type *__restrict__ p, size_t n, int lane) {
    using T = typename Elem<DT>::type;
    constexpr int E = Elem<DT>::E;
    size_t head = ((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / sizeof(T);
    head = head < n ? head : n;
    const size_t pieces = (n - head) / E, tail = head + pieces * E;
    double even = 0.0, odd = 0.0;
    if (static_cast<size_t>(lane) < head) {
        const double v = widen<DT>(p[lane]);
        even = __builtin_fma(v, v, even);
    }
    const uint4 *q = reinterpret_cast<const uint4 *>(p + head);
#pragma unroll FEWBIT_MOMENTS_UNROLL
    for (size_t c = lane; c < pieces; c += 64) {
        const uint4 w = q[c];
        const uint32_t word[4] = {w.x, w.y, w.z, w.w};
        if constexpr (E == 4) {
#pragma unroll
            for (int e = 0; e < 4; e += 2) {
                const double a = widen<DT>(word[e]), b = widen<DT>(word[e + 1]);
                even = __builtin_fma(a, a, even);
                odd = __builtin_fma(b, b, odd);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double a = widen<DT>(static_cast<T>(word[e] & 0xffffu)), b = widen<DT>(static_cast<T>(word[e] >> 16));
                even = __builtin_fma(a, a, even);
                odd = __builtin_fma(b, b, odd);
            }
        }
    }
    if (tail + lane < n) {
        const double v = widen<DT>(p[tail + lane]);
        odd = __builtin_fma(v, v, odd);
    }
    return wave_sum(even + odd);
}

// the workgroup's sums -> partial[3 * group + k], waves added in order (K values per wave)
template <int K> __device__ __forceinline__ void store_partials(const double (&mine)[K], double *__restrict__ partial, int lane, int wave) {
    __shared__ double of_wave[kWaves][K];
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) of_wave[wave][k] = mine[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double total = 0.0;
        if (threadIdx.x < K) {
            total = of_wave[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) total += of_wave[w][threadIdx.x];
        }
        partial[3 * static_cast<size_t>(blockIdx.x) + threadIdx.x] = total;
    }
}

template <int DX, int DG>
__global__ __launch_bounds__(kThreads) void row_moments_kernel(const void *__restrict__ x_, size_t n, size_t ldx, const void *__restrict__ g_, size_t m, size_t ldg,
                                                                size_t rows, size_t per_group, double *__restrict__ partial) {
    using TX = typename Elem<DX>::type;
    using TG = typename Elem<DG>::type;
    const TX *x = static_cast<const TX *>(x_);
    const TG *g = static_cast<const TG *>(g_);
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const size_t first = blockIdx.x * per_group, end = first + per_group < rows ? first + per_group : rows;
    double sum[3] = {0.0, 0.0, 0.0};
    for (size_t r = first + wave; r < end; r += kWaves) {
        const double xx = span_sum<DX>(x + r * ldx, n, lane), gg = span_sum<DG>(g + r * ldg, m, lane);
        sum[0] += xx;
        sum[1] += gg;
        sum[2] += xx * gg;
    }
    store_partials<3>(sum, partial, lane, wave);
}

template <int DT>
__global__ __launch_bounds__(kThreads) void sum_squares_kernel(const void *__restrict__ t_, size_t count, size_t pieces, size_t per_group, double *__restrict__ partial) {
    using T = typename Elem<DT>::type;
    const T *t = static_cast<const T *>(t_);
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const size_t first = blockIdx.x * per_group, end = first + per_group < pieces ? first + per_group : pieces;
    double sum[1] = {0.0};
    for (size_t c = first + wave; c < end; c += kWaves) {
        const size_t at = c * kPiece, len = count - at < kPiece ? count - at : kPiece;
        sum[0] += span_sum<DT>(t + at, len, lane);
    }
    store_partials<1>(sum, partial, lane, wave);
}

// one workgroup of 3 waves: wave k adds partial[3 i + k], i = 0 .. groups - 1 (lane l: i = l, l + 64, .. ascending; then the butterfly)
__global__ __launch_bounds__(192) void add_partials_kernel(const double *__restrict__ partial, size_t groups, int outputs, double *__restrict__ out) {
    const int lane = threadIdx.x % 64, k = threadIdx.x / 64;
    if (k >= outputs) return;
    double acc = 0.0;
    bool any = false;
    for (size_t i = lane; i < groups; i += 64) {
        const double v = partial[3 * i + k];
        acc = any ? acc + v : v;
        any = true;
    }
    acc = wave_sum(acc);
    if (lane == 0) out[k] = acc;
}

template <int DX> int launch_rows(int dtype_g, const void *x, size_t n, size_t ldx, const void *g, size_t m, size_t ldg, size_t rows, const Plan &p, double *partial,
                                  hipStream_t s) {
    const dim3 grid(static_cast<unsigned>(p.groups)), block(kThreads);
    switch (dtype_g) {
    case FEWBIT_F32: hipLaunchKernelGGL((row_moments_kernel<DX, FEWBIT_F32>), grid, block, 0, s, x, n, ldx, g, m, ldg, rows, p.per_group, partial); break;
    case FEWBIT_F16: hipLaunchKernelGGL((row_moments_kernel<DX, FEWBIT_F16>), grid, block, 0, s, x, n, ldx, g, m, ldg, rows, p.per_group, partial); break;
    default: hipLaunchKernelGGL((row_moments_kernel<DX, FEWBIT_BF16>), grid, block, 0, s, x, n, ldx, g, m, ldg, rows, p.per_group, partial); break;
    }
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : FEWBIT_ERR_LAUNCH;
}

inline int check_workspace(const char *name, const void *workspace, size_t workspace_bytes) {
    if (workspace == nullptr || workspace_bytes < kWorkspaceBytes || misaligned(workspace, 16))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: the workspace must be 16-byte aligned and hold fewbit_hipx_moments_workspace = %zu bytes (got %zu)", name,
                    kWorkspaceBytes, workspace_bytes);
    return FEWBIT_OK;
}

}  // namespace moments
}  // namespace fewbit_hip

using namespace fewbit_hip;
using namespace fewbit_hip::moments;

extern "C" {

size_t fewbit_hipx_moments_workspace(size_t rows, size_t n, size_t m) {
    if (rows == 0 || n == 0 || m == 0 || rows > kMaxRows || n > kMaxFeatures || m > kMaxFeatures) return 0;
    return kWorkspaceBytes;
}

int fewbit_hipx_row_moments(int dtype_x, const void *x, size_t n, size_t ldx, int dtype_g, const void *g, size_t m, size_t ldg, size_t rows, double *out3,
                            void *workspace, size_t workspace_bytes, void *stream) {
    if (!known_dtype(dtype_x)) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "row_moments: unknown dtype_x %d", dtype_x);
    if (!known_dtype(dtype_g)) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "row_moments: unknown dtype_g %d", dtype_g);
    if (rows == 0 || rows > kMaxRows) return fail(FEWBIT_ERR_UNSUPPORTED, "row_moments: rows = %zu has no kernel (1 .. %zu rows)", rows, kMaxRows);
    if (n == 0 || n > kMaxFeatures) return fail(FEWBIT_ERR_UNSUPPORTED, "row_moments: n = %zu has no kernel (1 .. %zu columns)", n, kMaxFeatures);
    if (m == 0 || m > kMaxFeatures) return fail(FEWBIT_ERR_UNSUPPORTED, "row_moments: m = %zu has no kernel (1 .. %zu columns)", m, kMaxFeatures);
    if (ldx < n) return fail(FEWBIT_ERR_UNSUPPORTED, "row_moments: ldx = %zu < n = %zu", ldx, n);
    if (ldg < m) return fail(FEWBIT_ERR_UNSUPPORTED, "row_moments: ldg = %zu < m = %zu", ldg, m);
    if (ldx > kMaxRows) return fail(FEWBIT_ERR_UNSUPPORTED, "row_moments: ldx = %zu is beyond %zu", ldx, kMaxRows);
    if (ldg > kMaxRows) return fail(FEWBIT_ERR_UNSUPPORTED, "row_moments: ldg = %zu is beyond %zu", ldg, kMaxRows);
    if (x == nullptr || g == nullptr || out3 == nullptr) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "row_moments: null pointer");
    if (misaligned(x, size_of(dtype_x)) || misaligned(g, size_of(dtype_g)) || misaligned(out3, 8))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "row_moments: x and g must be aligned to their element size, out3 to 8 bytes");
    if (const int rc = check_workspace("row_moments", workspace, workspace_bytes)) return rc;
    const Plan p = plan(rows, kMinRows);
    double *partial = static_cast<double *>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    switch (dtype_x) {
    case FEWBIT_F32: rc = launch_rows<FEWBIT_F32>(dtype_g, x, n, ldx, g, m, ldg, rows, p, partial, s); break;
    case FEWBIT_F16: rc = launch_rows<FEWBIT_F16>(dtype_g, x, n, ldx, g, m, ldg, rows, p, partial, s); break;
    default: rc = launch_rows<FEWBIT_BF16>(dtype_g, x, n, ldx, g, m, ldg, rows, p, partial, s); break;
    }
    if (rc != FEWBIT_OK) return fail(FEWBIT_ERR_LAUNCH, "row_moments: the launch failed");
    hipLaunchKernelGGL(add_partials_kernel, dim3(1), dim3(192), 0, s, partial, p.groups, 3, out3);
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "row_moments: the launch failed");
}

int fewbit_hipx_sum_squares(int dtype, const void *t, size_t count, double *out1, void *workspace, size_t workspace_bytes, void *stream) {
    if (!known_dtype(dtype)) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "sum_squares: unknown dtype %d", dtype);
    if (count == 0 || count > kMaxRows) return fail(FEWBIT_ERR_UNSUPPORTED, "sum_squares: count = %zu has no kernel (1 .. %zu elements)", count, kMaxRows);
    if (t == nullptr || out1 == nullptr) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "sum_squares: null pointer");
    if (misaligned(t, size_of(dtype)) || misaligned(out1, 8))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "sum_squares: t must be aligned to its element size, out1 to 8 bytes");
    if (const int rc = check_workspace("sum_squares", workspace, workspace_bytes)) return rc;
    const size_t pieces = (count + kPiece - 1) / kPiece;
    const Plan p = plan(pieces, kMinPieces);
    double *partial = static_cast<double *>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>(p.groups)), block(kThreads);
    switch (dtype) {
    case FEWBIT_F32: hipLaunchKernelGGL(sum_squares_kernel<FEWBIT_F32>, grid, block, 0, s, t, count, pieces, p.per_group, partial); break;
    case FEWBIT_F16: hipLaunchKernelGGL(sum_squares_kernel<FEWBIT_F16>, grid, block, 0, s, t, count, pieces, p.per_group, partial); break;
    default: hipLaunchKernelGGL(sum_squares_kernel<FEWBIT_BF16>, grid, block, 0, s, t, count, pieces, p.per_group, partial); break;
    }
    if (hipGetLastError() != hipSuccess) return fail(FEWBIT_ERR_LAUNCH, "sum_squares: the launch failed");
    hipLaunchKernelGGL(add_partials_kernel, dim3(1), dim3(192), 0, s, partial, p.groups, 1, out1);
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "sum_squares: the launch failed");
}

}  // extern "C"
