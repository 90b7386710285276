// fewbit_dropout.hip -- dropout whose mask is a FUNCTION of a 64-bit seed, on gfx950; part of the companion library libfewbit_hipx.so
// (include/fewbit_hipx.h, "the mask of a seed"):
//
//     out[i] = keep(first + i) ? round_to_dtype(float(src[i]) * scale [+ float(addend[i])]) : (addend ? addend[i] : +0)
//
// Forward (src = x) and backward (src = gy, no addend) are the same launch with the same seed: nothing is kept for backward but the seed.
// What it replaces: torch's dropout writes one bool per element in forward and reads it in backward (2 s + 1 bytes per element each way
// for an element of s bytes); here both passes move 2 s and evaluate Philox once per eight elements.
//
// ONE launch, no LDS, no workspace, no atomics.  Lanes run along the blocks of eight elements (one Philox call each); a lane's block is one
// 16-byte load and store for the 16-bit types and two for fp32 when every pointer is 16-byte aligned, element accesses otherwise and in the
// block that holds the tail -- the same arithmetic either way, so the same bytes.  A lane reads all of its block before it writes any of it:
// `out` may be `src` or `addend` exactly.  Plan (a pure function of n): blocks = ceil(n / 8), workgroups of 256 lanes, at most kMaxGroups of
// them; beyond that a lane sweeps on by the grid's width.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "fewbit_hipx.h"
#include "fewbit_philox.h"

#define FEWBIT_HIDDEN __attribute__((visibility("hidden")))

namespace fewbit_hip {
namespace dft {
FEWBIT_HIDDEN int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));          // fewbit_dft.hip (g_last_error)
}
namespace dropout {

using dft::fail;
using sketch::Key;

constexpr uint32_t kMaskDomain = 5u;        // counter word 3 (0 and 2: the dense sketches, 3: the sampled rows, 4: the CRS columns)
constexpr uint32_t kOne = 65536u;           // thresholds are in units of 2^-16
constexpr int kThreads = 256, kBlock = 8;   // lanes per workgroup; elements per Philox call
constexpr size_t kMaxGroups = 2048;         // one sweep of the grid: kMaxGroups * kThreads * kBlock = 2^22 elements

// the 16 bits of element e = i & 7 of a block: word e >> 1, low half for even e, high half for odd e
__host__ __device__ __forceinline__ uint32_t bits_of(const uint32_t (&w)[4], int e) { return (w[e >> 1] >> (16 * (e & 1))) & 0xffffu; }
__host__ __device__ __forceinline__ void block_words(uint64_t q, Key key, uint32_t (&w)[4]) {
    sketch::philox4x32(static_cast<uint32_t>(q), static_cast<uint32_t>(q >> 32), 0u, kMaskDomain, key, w);
}
inline float scale_of(uint32_t threshold) { return threshold < kOne ? static_cast<float>(65536.0 / static_cast<double>(kOne - threshold)) : 0.0f; }

inline bool known_dtype(int dtype) { return dtype == FEWBIT_F32 || dtype == FEWBIT_F16 || dtype == FEWBIT_BF16; }
inline size_t size_of(int dtype) { return dtype == FEWBIT_F32 ? 4 : 2; }

template <int DT> struct Elem { using type = uint16_t; };
template <> struct Elem<FEWBIT_F32> { using type = uint32_t; };

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

// one element: the product and the sum are fp32 values of their own, rounded once to the dtype
template <int DT, bool ADD>
__device__ __forceinline__ typename Elem<DT>::type one(typename Elem<DT>::type x, typename Elem<DT>::type r, bool keep, float scale) {
    float v = to_float<DT>(x) * scale;
    // (left to itself the compiler folds an fp16 operand's conversion, the arithmetic and the rounding to fp16 into one v_fma_mix*, which rounds
    // the exact result once: one step apart from torch's (x.float() * scale + r.float()).half() at the ties -- see fewbit_crs.hip)
    if constexpr (DT == FEWBIT_F16) asm("" : "+v"(v));
    if constexpr (ADD) {
        v = v + to_float<DT>(r);
        if constexpr (DT == FEWBIT_F16) asm("" : "+v"(v));
    }
    const typename Elem<DT>::type dropped = ADD ? r : typename Elem<DT>::type{0};
    return keep ? from_float<DT>(v) : dropped;
}

template <int DT> __device__ __forceinline__ void load8(const typename Elem<DT>::type *p, typename Elem<DT>::type (&v)[kBlock]) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    if constexpr (DT == FEWBIT_F32) {
        const uint4 a = q[0], b = q[1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        const uint4 a = q[0];
        const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int e = 0; e < kBlock; ++e) v[e] = static_cast<uint16_t>(w[e >> 1] >> (16 * (e & 1)));
    }
}
template <int DT> __device__ __forceinline__ void store8(typename Elem<DT>::type *p, const typename Elem<DT>::type (&v)[kBlock]) {
    uint4 *q = reinterpret_cast<uint4 *>(p);
    if constexpr (DT == FEWBIT_F32) {
        q[0] = uint4{v[0], v[1], v[2], v[3]};
        q[1] = uint4{v[4], v[5], v[6], v[7]};
    } else {
        q[0] = uint4{v[0] | static_cast<uint32_t>(v[1]) << 16, v[2] | static_cast<uint32_t>(v[3]) << 16, v[4] | static_cast<uint32_t>(v[5]) << 16,
                     v[6] | static_cast<uint32_t>(v[7]) << 16};
    }
}

// VEC: src, addend and out are 16-byte aligned, so every whole block is.  No __restrict__: out may be src or addend.
// q0 = first / 8, the block number of src[0] in the logical tensor.
template <int DT, bool ADD, bool VEC>
__global__ __launch_bounds__(kThreads) void dropout_kernel(const void *src_, const void *addend_, void *out_, size_t n, uint64_t q0, Key value, const Key *device,
                                                           uint32_t threshold, float scale) {
    using T = typename Elem<DT>::type;
    const T *src = static_cast<const T *>(src_), *addend = static_cast<const T *>(addend_);
    T *out = static_cast<T *>(out_);
    Key key = value;
    if (device != nullptr) key = *device;
    const size_t blocks = (n + kBlock - 1) / kBlock, width = static_cast<size_t>(gridDim.x) * kThreads;
    for (size_t b = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; b < blocks; b += width) {
        uint32_t w[4];
        block_words(q0 + b, key, w);
        const size_t i0 = b * kBlock;
        T x[kBlock], r[kBlock], y[kBlock];
        if (VEC && i0 + kBlock <= n) {
            load8<DT>(src + i0, x);
            if constexpr (ADD) load8<DT>(addend + i0, r);
#pragma unroll
            for (int e = 0; e < kBlock; ++e) y[e] = one<DT, ADD>(x[e], ADD ? r[e] : T{0}, bits_of(w, e) >= threshold, scale);
            store8<DT>(out + i0, y);
        } else {
            const int have = n - i0 < static_cast<size_t>(kBlock) ? static_cast<int>(n - i0) : kBlock;
#pragma unroll
            for (int e = 0; e < kBlock; ++e) {
                x[e] = e < have ? src[i0 + e] : T{0};
                if constexpr (ADD) r[e] = e < have ? addend[i0 + e] : T{0};
            }
#pragma unroll
            for (int e = 0; e < kBlock; ++e) y[e] = one<DT, ADD>(x[e], ADD ? r[e] : T{0}, bits_of(w, e) >= threshold, scale);
#pragma unroll
            for (int e = 0; e < kBlock; ++e)
                if (e < have) out[i0 + e] = y[e];
        }
    }
}

template <int DT, bool ADD>
void launch(bool vec, unsigned groups, hipStream_t s, const void *src, const void *addend, void *out, size_t n, uint64_t q0, Key key, const Key *device,
            uint32_t threshold, float scale) {
    if (vec) hipLaunchKernelGGL((dropout_kernel<DT, ADD, true>), dim3(groups), dim3(kThreads), 0, s, src, addend, out, n, q0, key, device, threshold, scale);
    else hipLaunchKernelGGL((dropout_kernel<DT, ADD, false>), dim3(groups), dim3(kThreads), 0, s, src, addend, out, n, q0, key, device, threshold, scale);
}

template <int DT>
void launch(bool add, bool vec, unsigned groups, hipStream_t s, const void *src, const void *addend, void *out, size_t n, uint64_t q0, Key key, const Key *device,
            uint32_t threshold, float scale) {
    if (add) launch<DT, true>(vec, groups, s, src, addend, out, n, q0, key, device, threshold, scale);
    else launch<DT, false>(vec, groups, s, src, addend, out, n, q0, key, device, threshold, scale);
}

}  // namespace dropout
}  // namespace fewbit_hip

using namespace fewbit_hip;
using namespace fewbit_hip::dropout;

extern "C" {

int fewbit_hipx_dropout_threshold(double p) {
    if (!(p >= 0.0 && p <= 1.0)) return -1;
    return static_cast<int>(std::nearbyint(p * 65536.0));             // (the product is exact; the default rounding mode: ties to even)
}

int fewbit_hipx_dropout_keep(uint64_t seed, uint32_t threshold, uint64_t first, size_t count, uint8_t *keep_host) {
    if (threshold > kOne) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "dropout_keep: threshold = %u is beyond 65536", threshold);
    if (count == 0) return FEWBIT_OK;
    if (keep_host == nullptr) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "dropout_keep: null pointer");
    if (first + count < first) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "dropout_keep: first + count exceeds 64 bits");
    const Key key = sketch::key_of(seed);
    uint32_t w[4];
    uint64_t have = ~uint64_t{0};
    for (size_t j = 0; j < count; ++j) {
        const uint64_t i = first + j;
        if ((i >> 3) != have || j == 0) {
            have = i >> 3;
            block_words(have, key, w);
        }
        keep_host[j] = bits_of(w, static_cast<int>(i & 7)) >= threshold;
    }
    return FEWBIT_OK;
}

int fewbit_hipx_dropout(int dtype, const void *src, const void *addend, void *out, size_t n, uint64_t first, uint64_t seed, const uint64_t *seed_device,
                        uint32_t threshold, void *stream) {
    if (!known_dtype(dtype)) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "dropout: unknown dtype %d", dtype);
    if (threshold > kOne) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "dropout: threshold = %u is beyond 65536", threshold);
    if ((first & 7) != 0) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "dropout: first = %llu is not a multiple of 8", static_cast<unsigned long long>(first));
    if (first + n < first) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "dropout: first + n exceeds 64 bits");
    if ((reinterpret_cast<uintptr_t>(seed_device) & 7) != 0) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "dropout: the seed word in device memory must be 8-byte aligned");
    if (n == 0) return FEWBIT_OK;
    if (src == nullptr || out == nullptr) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "dropout: null pointer");
    const uintptr_t all = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(addend) | reinterpret_cast<uintptr_t>(out);
    if (all % size_of(dtype) != 0) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "dropout: src, addend and out must be aligned to their element size");
    const size_t blocks = (n + kBlock - 1) / kBlock, wanted = (blocks + kThreads - 1) / kThreads;
    const unsigned groups = static_cast<unsigned>(wanted < kMaxGroups ? wanted : kMaxGroups);
    const bool vec = (all & 15) == 0;
    const Key key = sketch::key_of(seed);
    const Key *device = reinterpret_cast<const Key *>(seed_device);
    const float scale = scale_of(threshold);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
    case FEWBIT_F32: launch<FEWBIT_F32>(addend != nullptr, vec, groups, s, src, addend, out, n, first / kBlock, key, device, threshold, scale); break;
    case FEWBIT_F16: launch<FEWBIT_F16>(addend != nullptr, vec, groups, s, src, addend, out, n, first / kBlock, key, device, threshold, scale); break;
    default: launch<FEWBIT_BF16>(addend != nullptr, vec, groups, s, src, addend, out, n, first / kBlock, key, device, threshold, scale); break;
    }
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "dropout: the launch failed");
}

}  // extern "C"
