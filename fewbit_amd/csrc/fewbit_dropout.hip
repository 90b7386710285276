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
// `out` may be `src` or `addend` exactly.  Plan (a pure function of n; fewbit_unit.h, `sweep`, as fewbit_quant.hip's): blocks = ceil(n / 8),
// workgroups of 256 lanes, at most kMaxGroups of them; beyond that a lane sweeps on by the grid's width.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "fewbit_hipx.h"
#include "fewbit_philox.h"
#include "fewbit_quantdef.h"

namespace fewbit_hip {
namespace dropout {

// (the mask of a seed -- kMaskDomain, kOne, mask_bits, scale_of --, the plan and the refusals: fewbit_unit.h; Elem, load8, store8 and the Philox call
// of a block: fewbit_quantdef.h)
using namespace unit;
using namespace unit::sweep;
using quant::Elem;
using quant::load8;
using quant::store8;
using sketch::Key;

// (to_float / from_float are not fewbit_quantdef.h's widen / narrow: narrow<FEWBIT_F16> carries a barrier of its own and `one` places its own, so
// the fp16 kernels written with that pair grow by 33 to 56 instructions, EXPERIMENTS.md 8.27)
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

// one element: the product and the sum are fp32 values of their own, rounded once to the dtype (fewbit_norm.hip's dropped_sum / dropped_gradient are
// this on widen / narrow, and stay there: see above)
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
        quant::block_words<kMaskDomain>(q0 + b, key, w);                                            // (the packed form's call with the mask's counter word)
        const size_t i0 = b * kBlock;
        T x[kBlock], r[kBlock], y[kBlock];
        if (VEC && i0 + kBlock <= n) {
            load8<DT>(src + i0, x);
            if constexpr (ADD) load8<DT>(addend + i0, r);
#pragma unroll
            for (int e = 0; e < kBlock; ++e) y[e] = one<DT, ADD>(x[e], ADD ? r[e] : T{0}, mask_bits(w, e) >= threshold, scale);
            store8<DT>(out + i0, y);
        } else {
            const int have = n - i0 < static_cast<size_t>(kBlock) ? static_cast<int>(n - i0) : kBlock;
#pragma unroll
            for (int e = 0; e < kBlock; ++e) {
                x[e] = e < have ? src[i0 + e] : T{0};
                if constexpr (ADD) r[e] = e < have ? addend[i0 + e] : T{0};
            }
#pragma unroll
            for (int e = 0; e < kBlock; ++e) y[e] = one<DT, ADD>(x[e], ADD ? r[e] : T{0}, mask_bits(w, e) >= threshold, scale);
#pragma unroll
            for (int e = 0; e < kBlock; ++e)
                if (e < have) out[i0 + e] = y[e];
        }
    }
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
    if (keep_host == nullptr) return refuse_null("dropout_keep");
    if (first + count < first) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "dropout_keep: first + count exceeds 64 bits");
    const Key key = sketch::key_of(seed);
    uint32_t w[4];
    uint64_t have = ~uint64_t{0};
    for (size_t j = 0; j < count; ++j) {
        const uint64_t i = first + j;
        if ((i >> 3) != have || j == 0) {
            have = i >> 3;
            quant::block_words<kMaskDomain>(have, key, w);
        }
        keep_host[j] = mask_bits(w, static_cast<int>(i & 7)) >= threshold;
    }
    return FEWBIT_OK;
}

int fewbit_hipx_dropout(int dtype, const void *src, const void *addend, void *out, size_t n, uint64_t first, uint64_t seed, const uint64_t *seed_device,
                        uint32_t threshold, void *stream) {
    if (const int rc = check_dtype("dropout", dtype)) return rc;
    if (threshold > kOne) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "dropout: threshold = %u is beyond 65536", threshold);
    if ((first & 7) != 0) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "dropout: first = %llu is not a multiple of 8", static_cast<unsigned long long>(first));
    if (first + n < first) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "dropout: first + n exceeds 64 bits");
    if (const int rc = check_seed_word("dropout", seed_device)) return rc;
    if (n == 0) return FEWBIT_OK;
    if (src == nullptr || out == nullptr) return refuse_null("dropout");
    const auto all_aligned = [&](size_t to) { return !misaligned(src, to) && !misaligned(addend, to) && !misaligned(out, to); };
    if (!all_aligned(size_of(dtype))) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "dropout: src, addend and out must be aligned to their element size");
    const unsigned groups = grid_of((n + kBlock - 1) / kBlock);
    const Key key = sketch::key_of(seed);
    const Key *device = reinterpret_cast<const Key *>(seed_device);
    const float scale = scale_of(threshold);
    // (with and vec before without: the order in which the kernels are first named is their order in the device module, fewbit_quant.hip)
    pick_dtype(dtype, [&](auto dt) { pick<1, 0>(addend != nullptr, [&](auto add) { pick<1, 0>(all_aligned(16), [&](auto vec) {
        hipLaunchKernelGGL((dropout_kernel<decltype(dt)::value, decltype(add)::value != 0, decltype(vec)::value != 0>), dim3(groups), dim3(kThreads), 0,
                           static_cast<hipStream_t>(stream), src, addend, out, n, first / kBlock, key, device, threshold, scale);
    }); }); });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "dropout: the launch failed");
}

}  // extern "C"
