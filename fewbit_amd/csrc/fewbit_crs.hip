// fewbit_crs.hip -- column sampling of the weight gradient (LinearCRS, the reference's linear_crs) on gfx950, part of the companion
// library libfewbit_hipx.so (include/fewbit_hipx.h):
//
//     kept[r][j] = x[r][cols[j]] * scale[j]            forward: the drawn columns of the input, scaled     (crs_gather)
//     gw[o][c]   = pos[c] >= 0 ? t[o][pos[c]] : 0      backward: t = G^T kept spread over all of dL/dW      (crs_scatter)
//
// The columns are a FUNCTION of a 64-bit seed (definition: fewbit_hipx.h, "the columns of a seed"), evaluated by the host function
// fewbit_hipx_crs_columns and, with the same code, by the prep kernel below -- so nothing is drawn into memory by a launch of its own,
// nothing is read back to size the result, and with the seed in a device word a recorded launch draws fresh columns on every replay.
//
// What it replaces: randint + bincount + nonzero (a read-back and a stream synchronisation) + an indexed gather + a multiply in forward,
// zeros_like + an indexed assignment in backward.
//
// Two launches per entry point:
//   prep    one workgroup: counts the draws (LDS atomics up to kLdsCols columns, vector global atomics on the pos array beyond; integer
//           adds, so the order does not matter), one block scan compacts the hit columns in ascending order, and cols / scale / pos / m
//           go to the workspace.  cols[j] = -1 and scale[j] = 0 for m <= j < min(nopairs, in_features).
//   spread  ONE kernel for both directions: out[r][j] = idx[j] >= 0 ? src[r][idx[j]] (* scale[j]) : 0 for an rows x n contiguous `out`.
//           Lanes run along j, each lane owns the 16 bytes of `out` [j_lo, j_lo + E) of every row it serves (E = 4 fp32 / 8 16-bit
//           elements) and keeps its E indices and scales in registers for all of them; a wave serves 4 rows, a workgroup 16.  Since n
//           (= m in eager mode) is arbitrary, row r of `out` starts at any element offset: rows are dealt to workgroups by alignment
//           class (r mod P, P = E / gcd(n, E)), inside a class the 16-byte pieces of all rows sit at the same j, so every piece but
//           the first and last of a row is one aligned 16-byte store.  The reads are element gathers in ascending order: at the usual
//           density (39 % of the columns at nopairs = in_features / 2) neighbouring lanes share cache lines and every line of the
//           row is fetched once.  Bytes: rows x in_features in + rows x n out.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "fewbit_hipx.h"
#include "fewbit_philox.h"
#include "fewbit_unit.h"

namespace fewbit_hip {
namespace crs {

using unit::fail, unit::known_dtype, unit::misaligned, unit::check_dtype, unit::check_seed_word;
using sketch::Key;

constexpr uint32_t kColsDomain = 4u;        // counter word 3 (0 and 2: the dense sketches, 3: the sampled rows)
constexpr size_t kMaxCols = size_t{1} << 20, kMaxPairs = size_t{1} << 22;
constexpr int kPrepThreads = 1024, kLdsCols = 8192;
constexpr size_t kHeaderBytes = 16;         // m

// draw h of block q
__host__ __device__ __forceinline__ uint32_t drawn_col(uint32_t word, uint32_t in_features) {
    return static_cast<uint32_t>((static_cast<uint64_t>(word) * in_features) >> 32);
}
__host__ __device__ __forceinline__ float scale_of(int32_t count, uint32_t in_features, uint32_t nopairs) {
    return static_cast<float>(static_cast<double>(count) * static_cast<double>(in_features) / static_cast<double>(nopairs));
}

inline bool in_range(size_t in_features, size_t nopairs) { return in_features >= 1 && in_features <= kMaxCols && nopairs >= 1 && nopairs <= kMaxPairs; }
inline size_t round16(size_t b) { return (b + 15) / 16 * 16; }
inline size_t cap_max(size_t in_features, size_t nopairs) { return nopairs < in_features ? nopairs : in_features; }

struct Workspace {                          // [m | pos: int[in_features] | cols: int[cap_max] | scale: float[cap_max]], each 16-byte aligned
    int *m, *pos, *cols;
    float *scale;
    size_t bytes;
};
inline Workspace carve(void *base, size_t in_features, size_t nopairs) {
    uint8_t *p = static_cast<uint8_t *>(base);
    const size_t pos_bytes = round16(4 * in_features), cap_bytes = round16(4 * cap_max(in_features, nopairs));
    return Workspace{reinterpret_cast<int *>(p), reinterpret_cast<int *>(p + kHeaderBytes), reinterpret_cast<int *>(p + kHeaderBytes + pos_bytes),
                     reinterpret_cast<float *>(p + kHeaderBytes + pos_bytes + cap_bytes), kHeaderBytes + pos_bytes + 2 * cap_bytes};
}

// ---- prep: the columns of a seed, on the device ------------------------------------------------------------------------------------
// LDS: the counts live in LDS; otherwise in the pos array itself (zeroed, counted with vector global atomics, read back with atomic loads
// -- the adds are performed in L2, a plain load could be served an older line -- and overwritten with the position by the thread that read it).
template <bool LDS>
__global__ __launch_bounds__(kPrepThreads) void crs_prep_kernel(Key value, const Key *__restrict__ device, uint32_t in_features, uint32_t nopairs,
                                                                 int *__restrict__ m_out, int *__restrict__ pos, int *__restrict__ cols,
                                                                 float *__restrict__ scale) {
    __shared__ int lds_count[LDS ? kLdsCols : 1];
    __shared__ int wave_sum[kPrepThreads / 64];
    const int tid = threadIdx.x, lane = tid % 64, wave = tid / 64;
    Key key = value;
    if (device != nullptr) key = *device;
    int *count = LDS ? lds_count : pos;
    for (uint32_t c = tid; c < in_features; c += kPrepThreads) count[c] = 0;
    if constexpr (!LDS) __threadfence();
    __syncthreads();
    for (uint32_t q = tid; 4 * q < nopairs; q += kPrepThreads) {
        uint32_t w[4];
        sketch::philox4x32(q, 0u, 0u, kColsDomain, key, w);
#pragma unroll
        for (int h = 0; h < 4; ++h)
            if (4 * q + h < nopairs) atomicAdd(&count[drawn_col(w[h], in_features)], 1);
    }
    if constexpr (!LDS) __threadfence();
    __syncthreads();
    auto count_of = [&](uint32_t c) -> int {
        if constexpr (LDS) return count[c];
        else return __hip_atomic_load(&count[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    // thread t looks after the columns [t * chunk, (t + 1) * chunk): ascending in t, so an exclusive scan of the hit counts gives each
    // thread the position of its first hit column
    const uint32_t chunk = (in_features + kPrepThreads - 1) / kPrepThreads;
    const uint32_t c0 = tid * chunk < in_features ? tid * chunk : in_features, c1 = c0 + chunk < in_features ? c0 + chunk : in_features;
    int hits = 0;
    for (uint32_t c = c0; c < c1; ++c) hits += count_of(c) > 0;
    int incl = hits;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kPrepThreads / 64; ++w) {
        const int s = wave_sum[w];
        if (w < wave) before += s;
        total += s;
    }
    int j = before + incl - hits;
    for (uint32_t c = c0; c < c1; ++c) {
        const int n = count_of(c);
        if (n > 0) {
            cols[j] = static_cast<int>(c);
            scale[j] = scale_of(n, in_features, nopairs);
        }
        pos[c] = n > 0 ? j : -1;
        j += n > 0;
    }
    // the rest of the cap_max slots: no column
    const uint32_t cap = nopairs < in_features ? nopairs : in_features;
    for (uint32_t k = total + tid; k < cap; k += kPrepThreads) {
        cols[k] = -1;
        scale[k] = 0.0f;
    }
    if (tid == 0) *m_out = total;
}

// ---- spread: out[r][j] = idx[j] >= 0 ? src[r][idx[j]] (* scale[j]) : 0 ------------------------------------------------------------------
// (not fewbit_quantdef.h's Elem: E, the elements of a 16-byte piece; fewbit_moments.hip has the same)
template <int DT> struct Elem { using type = uint16_t; static constexpr int E = 8; };
template <> struct Elem<FEWBIT_F32> { using type = uint32_t; static constexpr int E = 4; };

template <int DT> __device__ __forceinline__ float to_float(typename Elem<DT>::type raw) {
    if constexpr (DT == FEWBIT_F32) return __builtin_bit_cast(float, raw);
    else if constexpr (DT == FEWBIT_BF16) return __builtin_bit_cast(float, static_cast<uint32_t>(raw) << 16);
    else return static_cast<float>(__builtin_bit_cast(_Float16, raw));
}
// round to nearest even, as torch's conversions do (a NaN becomes the canonical quiet NaN of the format)
template <int DT> __device__ __forceinline__ typename Elem<DT>::type from_float(float v) {
    if constexpr (DT == FEWBIT_F32) return __builtin_bit_cast(uint32_t, v);
    else if constexpr (DT == FEWBIT_BF16) {
        const uint32_t bits = __builtin_bit_cast(uint32_t, v);
        if (v != v) return static_cast<uint16_t>(0x7fc0u);
        return static_cast<uint16_t>((bits + 0x7fffu + ((bits >> 16) & 1u)) >> 16);
    } else return __builtin_bit_cast(uint16_t, static_cast<_Float16>(v));
}

constexpr int kSpreadThreads = 256, kWaveRows = 4, kGroupRows = (kSpreadThreads / 64) * kWaveRows;

// grid (row groups of all alignment classes, tiles of 64 pieces along j).  `classes` = P, `groups` = row groups per class; `limit`: the
// columns of src.
template <int DT, bool SCALED>
__global__ __launch_bounds__(kSpreadThreads) void crs_spread_kernel(const void *__restrict__ src_, size_t rows, size_t ld, const int *__restrict__ idx,
                                                                     const float *__restrict__ scale, int limit, size_t n, void *__restrict__ out_,
                                                                     unsigned classes, unsigned groups) {
    using T = typename Elem<DT>::type;
    constexpr int E = Elem<DT>::E;
    const T *src = static_cast<const T *>(src_);
    T *out = static_cast<T *>(out_);
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const size_t klass = blockIdx.x / groups, group = blockIdx.x % groups;
    // every row r = klass + classes * t of the class starts at the same offset from a 16-byte boundary: `head` elements lie before the first one
    const size_t start = reinterpret_cast<uintptr_t>(out) / sizeof(T) + klass * n;
    const int head = static_cast<int>((E - start % E) % E);
    const long long piece = static_cast<long long>(blockIdx.y) * 64 + lane;         // piece 0: the head [0, head), piece g: [head + (g - 1) E, head + g E)
    const long long j_lo = head + (piece - 1) * E;
    if (j_lo >= static_cast<long long>(n)) return;
    const bool whole = j_lo >= 0 && j_lo + E <= static_cast<long long>(n);
    int at[E];
    float factor[E];
    bool inside[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const long long j = j_lo + e;
        inside[e] = j >= 0 && j < static_cast<long long>(n);
        at[e] = inside[e] ? idx[j] : -1;
        at[e] = at[e] < limit ? at[e] : -1;                               // (a cap smaller than m: the columns of src that do not exist read as none)
        factor[e] = SCALED && inside[e] ? scale[j] : 0.0f;
    }
    const size_t t0 = group * kGroupRows + static_cast<size_t>(wave) * kWaveRows;
    T raw[kWaveRows][E];
    // every request of the wave's rows before the first is looked at (a clamped address instead of a guard: the loads stay unconditional)
#pragma unroll
    for (int i = 0; i < kWaveRows; ++i) {
        size_t r = klass + classes * (t0 + i);
        r = r < rows ? r : rows - 1;
#pragma unroll
        for (int e = 0; e < E; ++e) raw[i][e] = src[r * ld + static_cast<size_t>(at[e] >= 0 ? at[e] : 0)];
    }
#pragma unroll
    for (int i = 0; i < kWaveRows; ++i) {
        const size_t r = klass + classes * (t0 + i);
        if (r >= rows) break;
        T v[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            T one = raw[i][e];
            if constexpr (SCALED) {
                float product = to_float<DT>(one) * factor[e];
                // the fp32 product is a value of its own (the contract: rounded to fp32, then once to the dtype, as torch's (x.float() * scale).to(dtype)
                // does).  Left to itself the compiler folds an fp16 multiply and its conversion into one v_fma_mixlo_f16, which rounds the exact product
                // ONCE: one step apart wherever the fp32 rounding lands on a tie of fp16 (6 % of all patterns under scale 5/3).
                if constexpr (DT == FEWBIT_F16) asm("" : "+v"(product));
                one = from_float<DT>(product);
            }
            v[e] = at[e] >= 0 ? one : T{0};
        }
        T *dst = out + r * n + j_lo;
        if (whole) {
            uint4 q;
            if constexpr (E == 4) q = uint4{v[0], v[1], v[2], v[3]};
            else q = uint4{v[0] | static_cast<uint32_t>(v[1]) << 16, v[2] | static_cast<uint32_t>(v[3]) << 16, v[4] | static_cast<uint32_t>(v[5]) << 16,
                           v[6] | static_cast<uint32_t>(v[7]) << 16};
            *reinterpret_cast<uint4 *>(dst) = q;
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e)
                if (inside[e]) dst[e] = v[e];
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
inline int launch_prep(uint64_t seed, const uint64_t *seed_device, size_t in_features, size_t nopairs, const Workspace &ws, hipStream_t s) {
    const Key key = sketch::key_of(seed);
    const Key *device = reinterpret_cast<const Key *>(seed_device);
    const uint32_t in = static_cast<uint32_t>(in_features), np = static_cast<uint32_t>(nopairs);
    if (in_features <= static_cast<size_t>(kLdsCols))
        hipLaunchKernelGGL(crs_prep_kernel<true>, dim3(1), dim3(kPrepThreads), 0, s, key, device, in, np, ws.m, ws.pos, ws.cols, ws.scale);
    else
        hipLaunchKernelGGL(crs_prep_kernel<false>, dim3(1), dim3(kPrepThreads), 0, s, key, device, in, np, ws.m, ws.pos, ws.cols, ws.scale);
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : FEWBIT_ERR_LAUNCH;
}

template <int DT, bool SCALED>
int launch_spread(const void *src, size_t rows, size_t ld, const int *idx, const float *scale, size_t limit, size_t n, void *out, hipStream_t s) {
    constexpr size_t E = Elem<DT>::E;
    size_t g = n & (~n + 1);                                            // the lowest set bit of n: gcd(n, E) when capped at E
    g = g < E ? g : E;
    size_t classes = E / g;
    classes = classes < rows ? classes : rows;
    const size_t per_class = (rows + classes - 1) / classes, groups = (per_class + kGroupRows - 1) / kGroupRows;
    const size_t pieces = 2 + (n + E - 1) / E, tiles = (pieces + 63) / 64;
    if (classes * groups > 0x7fffffffu || tiles > 65535u) return fail(FEWBIT_ERR_UNSUPPORTED, "crs: %zu rows x %zu columns exceed the launch grid", rows, n);
    hipLaunchKernelGGL((crs_spread_kernel<DT, SCALED>), dim3(static_cast<unsigned>(classes * groups), static_cast<unsigned>(tiles)), dim3(kSpreadThreads), 0, s, src,
                       rows, ld, idx, scale, static_cast<int>(limit), n, out, static_cast<unsigned>(classes), static_cast<unsigned>(groups));
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "crs: the launch failed");
}

template <bool SCALED>
int spread(int dtype, const void *src, size_t rows, size_t ld, const int *idx, const float *scale, size_t limit, size_t n, void *out, hipStream_t s) {
    switch (dtype) {
    case FEWBIT_F32: return launch_spread<FEWBIT_F32, SCALED>(src, rows, ld, idx, scale, limit, n, out, s);
    case FEWBIT_F16: return launch_spread<FEWBIT_F16, SCALED>(src, rows, ld, idx, scale, limit, n, out, s);
    default: return launch_spread<FEWBIT_BF16, SCALED>(src, rows, ld, idx, scale, limit, n, out, s);
    }
}

// what both entry points check before anything is launched; -> FEWBIT_OK, or the status of the refusal
inline int check(const char *name, int dtype, size_t rows, size_t in_features, size_t nopairs, size_t cap, const uint64_t *seed_device, const void *workspace,
                 size_t workspace_bytes) {
    if (const int rc = check_dtype(name, dtype)) return rc;
    if (!in_range(in_features, nopairs))
        return fail(FEWBIT_ERR_UNSUPPORTED, "%s: in_features = %zu, nopairs = %zu has no kernel (1 .. %zu columns, 1 .. %zu pairs)", name, in_features, nopairs,
                    kMaxCols, kMaxPairs);
    if (rows == 0) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: no rows", name);
    if (cap == 0 || cap > cap_max(in_features, nopairs))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: cap = %zu is not in 1 .. min(nopairs, in_features) = %zu", name, cap, cap_max(in_features, nopairs));
    if (const int rc = check_seed_word(name, seed_device)) return rc;
    const size_t need = carve(nullptr, in_features, nopairs).bytes;
    if (workspace == nullptr || workspace_bytes < need || misaligned(workspace, 16))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: the workspace must be 16-byte aligned and hold fewbit_hipx_crs_workspace = %zu bytes (got %zu)", name, need,
                    workspace_bytes);
    return FEWBIT_OK;
}

}  // namespace crs
}  // namespace fewbit_hip

using namespace fewbit_hip;
using namespace fewbit_hip::crs;

extern "C" {

int fewbit_hipx_revision(void) { return FEWBIT_HIPX_REVISION; }

int fewbit_hipx_crs_columns(uint64_t seed, size_t in_features, size_t nopairs, int64_t *cols_host, int32_t *count_host, size_t *m) {
    if (!in_range(in_features, nopairs))
        return fail(FEWBIT_ERR_UNSUPPORTED, "crs_columns: in_features = %zu, nopairs = %zu is out of range (1 .. %zu columns, 1 .. %zu pairs)", in_features, nopairs,
                    kMaxCols, kMaxPairs);
    if (m == nullptr || (cols_host == nullptr) != (count_host == nullptr)) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "crs_columns: null pointer");
    const Key key = sketch::key_of(seed);
    std::vector<int32_t> count(in_features, 0);
    for (size_t q = 0; 4 * q < nopairs; ++q) {
        uint32_t w[4];
        sketch::philox4x32(static_cast<uint32_t>(q), 0u, 0u, kColsDomain, key, w);
        for (size_t h = 0; h < 4 && 4 * q + h < nopairs; ++h) ++count[drawn_col(w[h], static_cast<uint32_t>(in_features))];
    }
    size_t hit = 0;
    for (size_t c = 0; c < in_features; ++c) {
        if (count[c] == 0) continue;
        if (cols_host != nullptr) {
            cols_host[hit] = static_cast<int64_t>(c);
            count_host[hit] = count[c];
        }
        ++hit;
    }
    *m = hit;
    return FEWBIT_OK;
}

size_t fewbit_hipx_crs_workspace(int dtype, size_t rows, size_t in_features, size_t nopairs) {
    if (!known_dtype(dtype) || rows == 0 || !in_range(in_features, nopairs)) return 0;
    return carve(nullptr, in_features, nopairs).bytes;
}

int fewbit_hipx_crs_gather(int dtype, const void *x, size_t rows, size_t in_features, size_t ld, uint64_t seed, const uint64_t *seed_device, size_t nopairs, size_t cap,
                           void *out, void *workspace, size_t workspace_bytes, void *stream) {
    if (const int rc = check("crs_gather", dtype, rows, in_features, nopairs, cap, seed_device, workspace, workspace_bytes)) return rc;
    if (x == nullptr || out == nullptr) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "crs_gather: null pointer");
    if (ld < in_features) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "crs_gather: ld = %zu < in_features = %zu", ld, in_features);
    const Workspace ws = carve(workspace, in_features, nopairs);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (launch_prep(seed, seed_device, in_features, nopairs, ws, s) != FEWBIT_OK) return fail(FEWBIT_ERR_LAUNCH, "crs_gather: the launch failed");
    return spread<true>(dtype, x, rows, ld, ws.cols, ws.scale, in_features, cap, out, s);
}

int fewbit_hipx_crs_scatter(int dtype, const void *t, size_t out_features, size_t cap, uint64_t seed, const uint64_t *seed_device, size_t in_features, size_t nopairs,
                            void *gw, void *workspace, size_t workspace_bytes, void *stream) {
    if (const int rc = check("crs_scatter", dtype, out_features, in_features, nopairs, cap, seed_device, workspace, workspace_bytes)) return rc;
    if (t == nullptr || gw == nullptr) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "crs_scatter: null pointer");
    const Workspace ws = carve(workspace, in_features, nopairs);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (launch_prep(seed, seed_device, in_features, nopairs, ws, s) != FEWBIT_OK) return fail(FEWBIT_ERR_LAUNCH, "crs_scatter: the launch failed");
    return spread<false>(dtype, t, out_features, cap, ws.pos, nullptr, cap, in_features, gw, s);
}

}  // extern "C"
