// fewbit_quant.hip -- a tensor kept in 2, 4 or 8 bits per element with unbiased stochastic rounding, on gfx950; part of the companion library
// libfewbit_hipx.so (include/fewbit_hipx.h, "the packed form of a seed"):
//
//     group g = elements 64 g .. 64 g + 63 of the flat tensor: lo = min, step = (max - min) / L, L = 2^bits - 1
//     code(i) = min(L, floor((x[i] - lo) * inv + U(i))),  U(i) = 16 bits of Philox(seed, i) / 65536        decode: fma(code, step, lo)
//
// What QuantizedLinear (fewbit_amd/linear.py) keeps of its input for the weight gradient: every element, in a few bits, instead of a few rows
// or columns in full.  The packed form is a pure function of (values, bits, seed) that fewbit_hipx_quant_pack_host evaluates alike.
//
// Pack: ONE launch, no LDS, no workspace, no atomics.  Lanes run along the blocks of eight elements (one Philox call and one code word of
// `bits` bytes each); eight neighbouring lanes hold a group and reduce its minimum, maximum and poison flag with three DPP steps.  A
// lane's block is one 16-byte load for the 16-bit types and two for fp32 when src is 16-byte aligned, element loads otherwise and in the block
// that holds the tail -- the same arithmetic either way, so the same bytes.  Code words leave as one dword per lane pair (2 bits), per lane
// (4 bits) or two (8 bits), the parameters as 8 bytes from the first lane of a group: ordinary vector stores.
// Unpack: ONE launch; a lane reads its code word and its group's parameters and writes its block as 16-byte pieces.
// Plan of both (a pure function of n; fewbit_unit.h, `sweep`): blocks = ceil(n / 8), workgroups of 256 lanes (32 groups), at most kMaxGroups of
// them; beyond that a lane sweeps on by the grid's width.  The refusals the entry points share with the other units and the dispatcher that names
// the kernel of a call (pick) are fewbit_unit.h's too.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "fewbit_hipx.h"
#include "fewbit_philox.h"
#include "fewbit_quantdef.h"

#pragma clang fp contract(off)

namespace fewbit_hip {
namespace quant {

// (the definition itself -- lo, step, inv, code_of, decode, the poison rule, the rounding bits -- and the lane moves: fewbit_quantdef.h, the
// text fewbit_norm.hip evaluates too; the plan -- kThreads, kMaxGroups, grid_of -- and the refusals: fewbit_unit.h)
using namespace unit::sweep;

inline size_t bytes_of(size_t n, int bits) { return known_bits(bits) && n != 0 && n <= kMaxCount ? packed_bytes(n, bits) : 0; }

// VEC: src is 16-byte aligned, so every whole block is.  out: 8-byte aligned; the parameters of group g at 8 g, the code word of block b at
// 8 groups + BITS b.
template <int DT, int BITS, bool VEC>
__global__ __launch_bounds__(kThreads) void pack_kernel(const void *__restrict__ src_, size_t n, Key value, const Key *device, uint8_t *__restrict__ out) {
    using T = typename Elem<DT>::type;
    constexpr uint32_t kLevels = (1u << BITS) - 1u;
    const T *src = static_cast<const T *>(src_);
    Key key = value;
    if (device != nullptr) key = *device;
    const size_t blocks = (n + kBlock - 1) / kBlock, groups = (n + kGroup - 1) / kGroup, width = static_cast<size_t>(gridDim.x) * kThreads;
    uint8_t *codes = out + 8 * groups;
    // (the bound is a group's, not a block's: the eight lanes of a group leave the loop together, so every lane move below meets its partner)
    for (size_t b = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; b < groups * kLanes; b += width) {
        const size_t i0 = b * kBlock;
        const int have = b >= blocks ? 0 : n - i0 < static_cast<size_t>(kBlock) ? static_cast<int>(n - i0) : kBlock;
        T raw[kBlock];
        if (VEC && have == kBlock) {
            load8<DT>(src + i0, raw);
        } else {
            // (a missing element repeats the block's first, which moves neither the minimum, the maximum nor the flag, and its code is masked
            // away below: the arithmetic has no branch per element; a lane without elements holds zeros and is made neutral below)
#pragma unroll
            for (int e = 0; e < kBlock; ++e) raw[e] = e < have ? src[i0 + e] : e == 0 ? T{0} : raw[0];
        }
        uint32_t x[kBlock];
        int32_t kmin = INT32_MAX, kmax = INT32_MIN;
        uint32_t bad = 0;
#pragma unroll
        for (int e = 0; e < kBlock; ++e) {
            x[e] = widen<DT>(raw[e]);
            const int32_t k = order_key(x[e]);
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
            bad |= non_finite(x[e]) ? 1u : 0u;
        }
        if (have == 0) kmin = INT32_MAX, kmax = INT32_MIN, bad = 0;
        // lane ^ 1, lane ^ 2, then the other quad of the eight (mirrored: every lane of a quad holds the quad's result by then)
        reduce_step<kSwapPairs>(kmin, kmax, bad);
        reduce_step<kSwapHalves>(kmin, kmax, bad);
        reduce_step<kMirrorEight>(kmin, kmax, bad);
        const Params p = params_of(kmin, kmax, bad != 0, static_cast<float>(kLevels));
        uint32_t w[4];
        block_words(b, key, w);
        uint64_t word = 0;
#pragma unroll
        for (int e = 0; e < kBlock; ++e) word |= static_cast<uint64_t>(code_of(float_of_bits(x[e]), p, uniform_of(w, e), kLevels)) << (BITS * e);
        if (have < kBlock) word &= (uint64_t{1} << (BITS * have)) - 1;                              // the missing elements of the last word are 0
        if constexpr (BITS == 2) {
            // two lanes' words as one dword from the even lane; the last block of an odd count has no partner inside the buffer
            const uint32_t mine = static_cast<uint32_t>(word), other = static_cast<uint32_t>(lane_move<kSwapPairs>(static_cast<int>(mine)));
            if ((b & 1) == 0 && b + 1 < blocks) *reinterpret_cast<uint32_t *>(codes + 2 * b) = mine | other << 16;
            else if ((b & 1) == 0 && b < blocks) *reinterpret_cast<uint16_t *>(codes + 2 * b) = static_cast<uint16_t>(mine);
        } else if constexpr (BITS == 4) {
            if (b < blocks) *reinterpret_cast<uint32_t *>(codes + 4 * b) = static_cast<uint32_t>(word);
        } else {
            if (b < blocks) *reinterpret_cast<uint2 *>(codes + 8 * b) = uint2{static_cast<uint32_t>(word), static_cast<uint32_t>(word >> 32)};
        }
        if ((b & (kLanes - 1)) == 0) *reinterpret_cast<uint2 *>(out + 8 * (b / kLanes)) = uint2{bits_of_float(p.lo), bits_of_float(p.step)};
    }
}

template <int DT, int BITS, bool VEC>
__global__ __launch_bounds__(kThreads) void unpack_kernel(const uint8_t *__restrict__ packed, size_t n, void *__restrict__ out_) {
    using T = typename Elem<DT>::type;
    constexpr uint32_t kLevels = (1u << BITS) - 1u;
    T *out = static_cast<T *>(out_);
    const size_t blocks = (n + kBlock - 1) / kBlock, groups = (n + kGroup - 1) / kGroup, width = static_cast<size_t>(gridDim.x) * kThreads;
    const uint8_t *codes = packed + 8 * groups;
    for (size_t b = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; b < blocks; b += width) {
        const uint2 par = *reinterpret_cast<const uint2 *>(packed + 8 * (b / kLanes));
        uint64_t word;
        if constexpr (BITS == 2) word = *reinterpret_cast<const uint16_t *>(codes + 2 * b);
        else if constexpr (BITS == 4) word = *reinterpret_cast<const uint32_t *>(codes + 4 * b);
        else {
            const uint2 c = *reinterpret_cast<const uint2 *>(codes + 8 * b);
            word = c.x | static_cast<uint64_t>(c.y) << 32;
        }
        const float lo = float_of_bits(par.x), step = float_of_bits(par.y);
        T y[kBlock];
#pragma unroll
        for (int e = 0; e < kBlock; ++e) y[e] = narrow<DT>(decode(static_cast<uint32_t>(word >> (BITS * e)) & kLevels, lo, step));
        const size_t i0 = b * kBlock;
        if (VEC && i0 + kBlock <= n) {
            store8<DT>(out + i0, y);
        } else {
            const int have = n - i0 < static_cast<size_t>(kBlock) ? static_cast<int>(n - i0) : kBlock;
#pragma unroll
            for (int e = 0; e < kBlock; ++e)
                if (e < have) out[i0 + e] = y[e];
        }
    }
}

// f(dtype, bits, vec as compile-time constants) for the kernel of a call (vec before not: the order in which a unit first names its kernels is their
// order in the device module, and the code of the first and the last of them depends on it, EXPERIMENTS.md 8.27)
template <class F> void pick_kernel(int dtype, int bits, bool vec, F &&f) {
    pick_dtype(dtype, [&](auto dt) { pick<2, 4, 8>(bits, [&](auto b) { pick<1, 0>(vec, [&](auto v) { f(dt, b, v); }); }); });
}

// what the two host entry points refuse alike, the pointers last; 1: n = 0, nothing to do
inline int check_host(const char *name, int bits, size_t n, const void *from, const void *to) {
    if (const int rc = check_bits(name, bits)) return rc;
    if (n == 0) return 1;
    if (const int rc = check_count(name, n)) return rc;
    return from == nullptr || to == nullptr ? refuse_null(name) : FEWBIT_OK;
}

}  // namespace quant
}  // namespace fewbit_hip

using namespace fewbit_hip;
using namespace fewbit_hip::quant;

extern "C" {

size_t fewbit_hipx_quant_bytes(size_t n, int bits) { return bytes_of(n, bits); }

int fewbit_hipx_quant_pack_host(const float *x_host, size_t n, int bits, uint64_t seed, uint8_t *out_host) {
    if (const int rc = check_host("quant_pack_host", bits, n, x_host, out_host)) return rc < 0 ? rc : FEWBIT_OK;
    const size_t groups = (n + kGroup - 1) / kGroup;
    const Key key = sketch::key_of(seed);
    uint8_t *codes = out_host + 8 * groups;
    // (group g starts at block kLanes g of the flat tensor)
    for (size_t g = 0; g < groups; ++g) {
        const size_t first = g * kGroup, count = n - first < static_cast<size_t>(kGroup) ? n - first : kGroup;
        pack_group_host(x_host + first, count, g * kLanes, key, bits, out_host + 8 * g, codes + static_cast<size_t>(bits) * kLanes * g);
    }
    return FEWBIT_OK;
}

int fewbit_hipx_quant_unpack_host(const uint8_t *packed_host, size_t n, int bits, float *out_host) {
    if (const int rc = check_host("quant_unpack_host", bits, n, packed_host, out_host)) return rc < 0 ? rc : FEWBIT_OK;
    const uint8_t *codes = packed_host + 8 * ((n + kGroup - 1) / kGroup);
    for (size_t i = 0; i < n; ++i) out_host[i] = decode_host(packed_host, codes, i, bits);
    return FEWBIT_OK;
}

int fewbit_hipx_quant_pack(int dtype, const void *src, size_t n, int bits, uint64_t seed, const uint64_t *seed_device, uint8_t *out, size_t out_bytes,
                           void *stream) {
    const char *name = "quant_pack";
    if (const int rc = check_dtype(name, dtype)) return rc;
    if (const int rc = check_bits(name, bits)) return rc;
    if (const int rc = check_seed_word(name, seed_device)) return rc;
    if (n == 0) return FEWBIT_OK;
    if (const int rc = check_count(name, n)) return rc;
    if (src == nullptr || out == nullptr) return refuse_null(name);
    if (misaligned(src, size_of(dtype))) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "quant_pack: src must be aligned to its element size");
    if (const int rc = check_aligned8(name, "out", out)) return rc;
    if (const int rc = check_bytes(name, "out", out_bytes, bytes_of(n, bits))) return rc;
    const unsigned grid = grid_of((n + kGroup - 1) / kGroup * kLanes);
    const Key key = sketch::key_of(seed);
    const Key *device = reinterpret_cast<const Key *>(seed_device);
    pick_kernel(dtype, bits, !misaligned(src, 16), [&](auto dt, auto b, auto v) {
        hipLaunchKernelGGL((pack_kernel<dt(), b(), v() != 0>), dim3(grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream), src, n, key, device, out);
    });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "quant_pack: the launch failed");
}

int fewbit_hipx_quant_unpack(const uint8_t *packed, size_t n, int bits, int out_dtype, void *out, void *stream) {
    const char *name = "quant_unpack";
    if (const int rc = check_dtype(name, out_dtype)) return rc;
    if (const int rc = check_host(name, bits, n, packed, out)) return rc < 0 ? rc : FEWBIT_OK;
    if (const int rc = check_aligned8(name, "packed", packed)) return rc;
    if (misaligned(out, size_of(out_dtype))) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "quant_unpack: out must be aligned to its element size");
    const unsigned grid = grid_of((n + kBlock - 1) / kBlock);
    pick_kernel(out_dtype, bits, !misaligned(out, 16), [&](auto dt, auto b, auto v) {
        hipLaunchKernelGGL((unpack_kernel<dt(), b(), v() != 0>), dim3(grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream), packed, n, out);
    });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "quant_unpack: the launch failed");
}

}  // extern "C"
