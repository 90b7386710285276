// fewbit_quantdef.h -- the definition of "the packed form of a seed" (include/fewbit_hipx.h), one element or one group at a time: the ONE text
// that fewbit_quant.hip (a tensor taken by flat index) and fewbit_norm.hip (the normalized rows of a layer norm) evaluate, on the host and
// on the device alike.  Also the element access and the lane moves both units share (fewbit_dropout.hip: the element access; fewbit_glu.hip: all of it).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "fewbit_hipx.h"
#include "fewbit_philox.h"
#include "fewbit_unit.h"

namespace fewbit_hip {
namespace quant {

using namespace unit;                       // (the predicates, the refusals, pick)
using unit::kBlock, unit::kGroup, unit::kLanes;        // (declared here: fewbit_device.h has a kBlock of its own in fewbit_hip)
using sketch::Key;

constexpr uint32_t kRoundDomain = 7u;       // counter word 3 (0 and 2: the dense sketches, 3: the sampled rows, 4: the CRS columns, 5: the dropout, 6: the signs)
constexpr uint32_t kNaN = 0x7fc00000u;      // what a poisoned group stores for lo and step, and decodes to

// ---- the definition, one element or one group at a time: host and device evaluate these very functions --------------------------------------
// each is ONE correctly rounded fp32 operation (the device intrinsics keep the compiler from contracting a pair of them; the host is
// compiled with contraction off)
__host__ __device__ __forceinline__ float sub_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(a, b);
#else
    return a - b;
#endif
}
__host__ __device__ __forceinline__ float mul_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;
#endif
}
__host__ __device__ __forceinline__ float add_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}
__host__ __device__ __forceinline__ float div_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}
__host__ __device__ __forceinline__ float fma_rn(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmaf_rn(a, b, c);
#else
    return std::fmaf(a, b, c);
#endif
}

__host__ __device__ __forceinline__ uint32_t bits_of_float(float v) { return __builtin_bit_cast(uint32_t, v); }
__host__ __device__ __forceinline__ float float_of_bits(uint32_t b) { return __builtin_bit_cast(float, b); }

// the order of the reals on the bits of a finite float, -0 below +0, as a signed integer (its own inverse)
__host__ __device__ __forceinline__ int32_t order_key(uint32_t bits) {
    return static_cast<int32_t>(bits ^ (static_cast<uint32_t>(static_cast<int32_t>(bits) >> 31) & 0x7fffffffu));
}
__host__ __device__ __forceinline__ bool non_finite(uint32_t bits) { return (bits & 0x7f800000u) == 0x7f800000u; }

// the 16 bits of element e of a block (the dropout's choice: mask_bits, fewbit_unit.h) as U in [0, 1)
__host__ __device__ __forceinline__ float uniform_of(const uint32_t (&w)[4], int e) {
    return static_cast<float>(mask_bits(w, e)) * (1.0f / 65536.0f);                                     // (both exact)
}
// (DOMAIN: counter word 3, a compile-time constant as it always was; kUpDomain is the second tensor of a call that packs two, fewbit_glu.hip)
constexpr uint32_t kUpDomain = 8u;
template <uint32_t DOMAIN = kRoundDomain> __host__ __device__ __forceinline__ void block_words(uint64_t q, Key key, uint32_t (&w)[4]) {
    sketch::philox4x32(static_cast<uint32_t>(q), static_cast<uint32_t>(q >> 32), 0u, DOMAIN, key, w);
}

struct Params { float lo, step, inv; bool poisoned; };

// from the keys of a group's minimum and maximum and whether it holds a NaN or an infinity
__host__ __device__ __forceinline__ Params params_of(int32_t kmin, int32_t kmax, bool bad, float levels) {
    Params p;
    p.lo = float_of_bits(static_cast<uint32_t>(order_key(static_cast<uint32_t>(kmin))));
    const float hi = float_of_bits(static_cast<uint32_t>(order_key(static_cast<uint32_t>(kmax))));
    const float range = sub_rn(hi, p.lo);
    p.poisoned = bad || non_finite(bits_of_float(range));
    if (p.poisoned) {
        p.lo = p.step = float_of_bits(kNaN);
        p.inv = 0.0f;
        return p;
    }
    p.step = div_rn(range, levels);
    const float inv = range > 0.0f ? div_rn(levels, range) : 0.0f;
    p.inv = non_finite(bits_of_float(inv)) ? 0.0f : inv;              // (a range below L / FLT_MAX: every code is 0, see the header)
    return p;
}
__host__ __device__ __forceinline__ uint32_t code_of(float x, const Params &p, float u, uint32_t levels) {
    if (p.poisoned) return 0u;
    const float t = mul_rn(sub_rn(x, p.lo), p.inv);
    const uint32_t c = static_cast<uint32_t>(floorf(add_rn(t, u)));    // (0 <= t + u < L + 2: the conversion is exact)
    return c < levels ? c : levels;
}
__host__ __device__ __forceinline__ float decode(uint32_t code, float lo, float step) {
    if (step != step) return float_of_bits(kNaN);
    return fma_rn(static_cast<float>(code), step, lo);
}

// ---- the host evaluation, one group or one element at a time: what the four *_host entry points loop over -----------------------------------
// the `count` (1 .. kGroup) values of a group whose first block is block `first_block` of the seed's stream -> its 8 parameter bytes (lo, step,
// little-endian) and its bits * ceil(count / 8) code bytes (the missing elements of the last word are 0)
template <uint32_t DOMAIN = kRoundDomain>
inline void pack_group_host(const float *x, size_t count, uint64_t first_block, Key key, int bits, uint8_t *params, uint8_t *codes) {
    const uint32_t levels = (1u << bits) - 1u;
    int32_t kmin = INT32_MAX, kmax = INT32_MIN;
    bool bad = false;
    for (size_t j = 0; j < count; ++j) {
        const uint32_t bits32 = bits_of_float(x[j]);
        const int32_t k = order_key(bits32);
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
        bad = bad || non_finite(bits32);
    }
    const Params p = params_of(kmin, kmax, bad, static_cast<float>(levels));
    const uint32_t par[2] = {bits_of_float(p.lo), bits_of_float(p.step)};
    for (int h = 0; h < 2; ++h)
        for (int c = 0; c < 4; ++c) params[4 * h + c] = static_cast<uint8_t>(par[h] >> (8 * c));
    for (size_t j0 = 0; j0 < count; j0 += kBlock) {
        uint32_t w[4];
        block_words<DOMAIN>(first_block + j0 / kBlock, key, w);
        uint64_t word = 0;
        for (int e = 0; e < kBlock && j0 + e < count; ++e) word |= static_cast<uint64_t>(code_of(x[j0 + e], p, uniform_of(w, e), levels)) << (bits * e);
        for (int c = 0; c < bits; ++c) codes[static_cast<size_t>(bits) * (j0 / kBlock) + c] = static_cast<uint8_t>(word >> (8 * c));
    }
}
// element i of a run of groups: `params` the parameter bytes of its first group, `codes` the code bytes of its first block
inline float decode_host(const uint8_t *params, const uint8_t *codes, size_t i, int bits) {
    uint32_t par[2] = {0, 0};
    for (int h = 0; h < 2; ++h)
        for (int c = 0; c < 4; ++c) par[h] |= static_cast<uint32_t>(params[8 * (i / kGroup) + 4 * h + c]) << (8 * c);
    const size_t bit = static_cast<size_t>(bits) * (i % kBlock);
    const uint32_t code = (codes[static_cast<size_t>(bits) * (i / kBlock) + bit / 8] >> (bit % 8)) & ((1u << bits) - 1u);
    return decode(code, float_of_bits(par[0]), float_of_bits(par[1]));
}

inline bool known_bits(int bits) { return bits == 2 || bits == 4 || bits == 8; }
// (the refusal of the others, beside those of fewbit_unit.h)
inline int check_bits(const char *name, int bits) {
    return known_bits(bits) ? FEWBIT_OK : fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: bits = %d is not 2, 4 or 8", name, bits);
}

// ---- element access ----------------------------------------------------------------------------------------------------------------------
template <int DT> struct Elem { using type = uint16_t; };
template <> struct Elem<FEWBIT_F32> { using type = uint32_t; };

// (widen / narrow are not fewbit_dropout.hip's to_float / from_float: narrow<FEWBIT_F16> carries the barrier that `one` places itself there, and either
// unit written with the other's pair changes its fp16 kernels, EXPERIMENTS.md 8.27)
template <int DT> __device__ __forceinline__ uint32_t widen(typename Elem<DT>::type raw) {              // the bits of the element as fp32 (exact)
    if constexpr (DT == FEWBIT_F32) return raw;
    else if constexpr (DT == FEWBIT_BF16) return static_cast<uint32_t>(raw) << 16;
    else return bits_of_float(static_cast<float>(__builtin_bit_cast(_Float16, raw)));
}
// round to nearest even, as torch's conversions do (a NaN becomes the canonical quiet NaN of the format)
template <int DT> __device__ __forceinline__ typename Elem<DT>::type narrow(float v) {
    if constexpr (DT == FEWBIT_F32) return bits_of_float(v);
    else if constexpr (DT == FEWBIT_BF16) {
        const uint32_t bits = bits_of_float(v);
        if (v != v) return static_cast<uint16_t>(0x7fc0u);
        return static_cast<uint16_t>((bits + 0x7fffu + ((bits >> 16) & 1u)) >> 16);
    } else {
        // (left to itself the compiler folds the fma and the rounding to fp16 into one v_fma_mix*, which rounds the exact result once)
        asm("" : "+v"(v));
        return __builtin_bit_cast(uint16_t, static_cast<_Float16>(v));
    }
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

// Data-parallel-primitive moves inside a row of 16 lanes (no LDS crossbar): quad_perm [1, 0, 3, 2], quad_perm [2, 3, 0, 1], row_half_mirror.
// The eight lanes of a group are active together, so every source lane is.
constexpr int kSwapPairs = 0xB1, kSwapHalves = 0x4E, kMirrorEight = 0x141;
template <int CTRL> __device__ __forceinline__ int lane_move(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false); }
template <int CTRL> __device__ __forceinline__ void reduce_step(int32_t &kmin, int32_t &kmax, uint32_t &bad) {
    const int32_t omin = lane_move<CTRL>(kmin), omax = lane_move<CTRL>(kmax);
    bad |= static_cast<uint32_t>(lane_move<CTRL>(static_cast<int>(bad)));
    kmin = omin < kmin ? omin : kmin;
    kmax = omax > kmax ? omax : kmax;
}

}  // namespace quant
}  // namespace fewbit_hip
