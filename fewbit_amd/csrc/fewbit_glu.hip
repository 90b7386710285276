// fewbit_glu.hip -- the product of a gated MLP, y = act(gate) * up, that keeps BOTH inputs in 2, 4 or 8 bits per element for backward, on gfx950;
// part of the companion library libfewbit_hipx.so (include/fewbit_hipx.h, "the gate and the up of a seed"):
//
//     y[i]   = round_to_dtype(act(g) * u)                                   act: silu or gelu (erf), the functors of fewbit_device.h (16-bit I/O: gelu_relative, sigmoid_relative)
//     state  = [the packed form of the seed of gate | zero bytes up to a multiple of 8 | the same of up with counter word 3 = 8 | zero bytes]
//     d_up   = round(gy * act(g^)),  d_gate = round((gy * u^) * act'(g^))   g^, u^: the decodes
//
// What QuantizedGLU (fewbit_amd/glu.py) keeps instead of gate, act(gate) and up.  The state is a pure function of (values, bits, seed) that
// fewbit_hipx_glu_state_host evaluates alike; its two parts are the definition of fewbit_quantdef.h, the text fewbit_quant.hip evaluates.
//
// Forward: ONE launch, no LDS, no workspace, no atomics.  The plan is fewbit_quant.hip's: lanes run along the blocks of eight FLAT elements
// i = r * width + c of both inputs (two Philox calls, two code words and 16 bytes of y each; 32 bytes of y for fp32); eight neighbouring lanes
// hold a group of each input and reduce both minima, maxima and poison flags with three DPP steps.  A lane's block is 16-byte accesses where the
// width is a multiple of 8 (a block never straddles two rows then) and every base and row stride is 16-byte aligned, element accesses with (r, c)
// from the flat index otherwise: the same arithmetic either way, so the same bytes.  The gap between `width` and a row stride is never touched.
// Backward: ONE launch; a lane reads its two code words, the parameters of its two groups and its block of gy and writes its blocks of d_gate and
// d_up (either may be absent).  The same launch with PRODUCT set (fewbit_hipx_glu_backward_product) also writes act(g^) * u^, the product rebuilt from
// the decodes: what the gated MLP as one node (fewbit_amd/glu.py, gated_mlp_quantized) feeds to the weight gradient of down_proj instead of a kept y.
// One unit per dtype (-DFEWBIT_GLU_TU=0 / 1 / 2: fp32 with the C entry points, fp16, bf16), compiled in parallel and linked into one library.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "fewbit_device.h"
#include "fewbit_hipx.h"
#include "fewbit_philox.h"
#include "fewbit_quantdef.h"

#pragma clang fp contract(off)

namespace fewbit_hip {
namespace quant {
namespace glu {

using namespace unit;                       // (named again for the entry points below, which speak of glu::)
using namespace unit::sweep;                // the plan of fewbit_quant.hip: kThreads, kMaxGroups, grid_of (fewbit_unit.h)

struct ForwardArgs {
    const void *gate, *up;
    size_t ld_gate, ld_up, width, n;
    Key key;
    const Key *device;
    void *y;
    uint8_t *state;                         // nullptr: the plain forward (BITS = 0)
    size_t part;                            // bytes of one part of the state, padding included
};
struct BackwardArgs {
    const void *gy;
    const uint8_t *state;
    size_t part, width, n;
    void *d_gate, *d_up;
    size_t ld_dgate, ld_dup;
};
struct ProductArgs : BackwardArgs {         // the PRODUCT kernels: a third output; gy may then be nullptr where d_gate and d_up both are
    void *product;
    size_t ld_product;
};

// ---- where flat index i lies in a matrix of `width` columns whose rows are `ld` elements apart ---------------------------------------------------
struct Where { size_t r, c; };
// (`small`: n < 2^32, the same in every lane; the 64-bit division is some forty instructions longer)
__device__ __forceinline__ Where where_of(size_t i, size_t width, bool small) {
    if (small) {
        const uint32_t r = static_cast<uint32_t>(i) / static_cast<uint32_t>(width);
        return Where{r, static_cast<uint32_t>(i) - r * static_cast<uint32_t>(width)};
    }
    const size_t r = i / width;
    return Where{r, i - r * width};
}

// the `have` (0 .. 8) elements from flat index i0 = (at.r, at.c) on.  VEC: width % 8 == 0 and base and stride are 16-byte aligned, so a whole
// block lies in one row at a 16-byte aligned address.  A missing element repeats the block's first (fewbit_quant.hip).
template <int DT, bool VEC>
__device__ __forceinline__ void load_rows(const typename Elem<DT>::type *base, size_t ld, size_t width, Where at, int have, typename Elem<DT>::type (&raw)[kBlock]) {
    using T = typename Elem<DT>::type;
    size_t off = at.r * ld + at.c, c = at.c;
    if (VEC && have == kBlock) {
        load8<DT>(base + off, raw);
        return;
    }
#pragma unroll
    for (int e = 0; e < kBlock; ++e) {
        if (e < have) {
            raw[e] = base[off];
            ++off;
            if (++c == width) c = 0, off += ld - width;                 // (the next row; the gap is stepped over, never read)
        } else {
            raw[e] = e == 0 ? T{0} : raw[0];
        }
    }
}
template <int DT, bool VEC>
__device__ __forceinline__ void store_rows(typename Elem<DT>::type *base, size_t ld, size_t width, Where at, int have, const typename Elem<DT>::type (&raw)[kBlock]) {
    size_t off = at.r * ld + at.c, c = at.c;
    if (VEC && have == kBlock) {
        store8<DT>(base + off, raw);
        return;
    }
#pragma unroll
    for (int e = 0; e < kBlock; ++e) {
        if (e < have) {
            base[off] = raw[e];
            ++off;
            if (++c == width) c = 0, off += ld - width;
        }
    }
}

// ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------------------
// gelu to a few fp32 ulps RELATIVE to its value on the whole line.  Both classes of fewbit_device.h are accurate relative to |g| only: gelu_fast holds
// Phi(-|g|) to 4.5e-8 absolute and g 0.5 (1 + erf(g / sqrt 2)) cancels in 1 + erf, so below g = -2 either loses the value itself -- nothing a 16-bit
// gelu sees, but here the value is multiplied by `up` and the product is held to half an ulp of ITSELF.  So:
//   g >= -1/2 : the precise class's formula (1 + erf >= 0.61: no cancellation to speak of)
//   g <  -1/2 : g * 0.5 * erfc(z), z = -g / sqrt 2 as zh + zl (the rounding error of the product fed back: d log erfc / dz is about -2 z, and
//               z * 2^-24 of it would cost 2 z^2 * 2^-24 of the value, 10^-5 at g = -13), erfc(zh + zl) = erfc(zh) (1 - rho(zh) zl) with
//               rho = (2 / sqrt pi) exp(-z^2) / erfc(z) = 2 z + 1 / (z + 1 / z) to 2 % from z = 2 on (40 % at z = 0.35, of a term of 3e-8)
__device__ __forceinline__ float gelu_relative(float g) {
    constexpr float kHi = 0.707106769084930419921875f, kLo = 1.2101617e-08f;                         // fp32(1 / sqrt 2) and what it leaves of 1 / sqrt 2
    const float head = Act<FEWBIT_GELU, false>::eval(g, 0.0f, 0.0f);
    const float a = -g;
    const float zh = mul_rn(a, kHi);
    const float zl = add_rn(fma_rn(a, kHi, -zh), mul_rn(a, kLo));
    const float p = erfcf(zh);
    const float rho = add_rn(mul_rn(2.0f, zh), __builtin_amdgcn_rcpf(add_rn(zh, __builtin_amdgcn_rcpf(zh))));
    // (erfc is below the smallest fp32 from z = 10.06 on: the value is -0, as in float64, also where zh has overflowed and zl is a NaN)
    const float tail = zh > 10.1f ? 0.0f : fma_rn(-p, mul_rn(rho, zl), p);
    return g < -0.5f ? mul_rn(g, mul_rn(0.5f, tail)) : head;
}

// sigmoid to a few fp32 ulps RELATIVE to its value on the whole line, as a scaled pair: sigmoid(g) = m * scale, 1 - sigmoid(g) = rest.  The fast
// class's sigmoid_fast is rcp(1 + exp2(g * -log2e)): the one rounding of the argument costs |g| 2^-24 of exp(-g), which below g = -16 is more of
// sigmoid(g) than the 2^-20 a product is allowed, and from g = -87.4 down the reciprocal is an fp32 subnormal that v_rcp_f32 gives as 0, while
// silu(g) stays a normal bf16 number down to g = -97 and a subnormal one down to g = -105 (every bf16 gate, tests/test_gpu_glu_values.py).  So:
//   the argument   t log2e as uh + ul, t = -g clamped to [-128, 256] (beyond: sigmoid is 1, or below every fp32 number; no inf - inf in ul),
//                  the rounding error of the product and what fp32(log2 e) leaves of log2 e fed back: exp(-g) = exp2(uh) (1 + ul ln 2)
//   g >= -64     : m = rcp(1 + e) (1 - ul ln 2 (1 - m)), scale = 1, rest = 1 - m
//   g <  -64     : 1 + e is e in fp32 (e > 2^92): m = rcp(exp2(uh - 64)) (1 - ul ln 2), a normal number down to g = -131, scale = 2^-64, rest = 1.
//                  The caller multiplies by the scale LAST, so that the one product that enters the subnormals is rounded once.
struct Sigmoid { float m, scale, rest; };
__device__ __forceinline__ Sigmoid sigmoid_relative(float g) {
    constexpr float kHi = 1.44269502162933349609375f, kLo = 1.92596299112661746e-08f;                 // fp32(log2 e) and what it leaves of log2 e
    const bool far = g < -64.0f;
    const float t = __builtin_fminf(__builtin_fmaxf(-g, -128.0f), 256.0f);
    const float uh = mul_rn(t, kHi);
    const float ul = add_rn(fma_rn(t, kHi, -uh), mul_rn(t, kLo));
    const float e = __builtin_amdgcn_exp2f(far ? sub_rn(uh, 64.0f) : uh);
    const float m0 = __builtin_amdgcn_rcpf(far ? e : add_rn(1.0f, e));
    const float rest0 = sub_rn(1.0f, m0);
    const float m = fma_rn(-m0, mul_rn(mul_rn(ul, kLn2), far ? 1.0f : rest0), m0);
    return Sigmoid{m, far ? 0x1p-64f : 1.0f, far ? 1.0f : sub_rn(1.0f, m)};
}

// act in fp32.  silu: the precise class for fp32 I/O; g * sigmoid_relative(g) for 16-bit I/O.  gelu: the precise class for fp32 I/O (ATen's
// formula, and the check of fp32 is against ATen); gelu_relative for 16-bit I/O
template <int ACT, bool FAST> __device__ __forceinline__ float act_of(float g) {
    if constexpr (ACT == FEWBIT_GELU && FAST) return gelu_relative(g);
    else if constexpr (ACT == FEWBIT_SILU && FAST) {
        const Sigmoid s = sigmoid_relative(g);
        return mul_rn(mul_rn(g, s.m), s.scale);
    } else return Act<ACT, FAST>::eval(g, 0.0f, 0.0f);
}

// act' in fp32, one operation per step:  silu: s (1 + g (1 - s)), s = sigmoid(g);  gelu: Phi(g) + g phi(g)
template <int ACT, bool FAST> __device__ __forceinline__ float slope_of(float g) {
    if constexpr (ACT == FEWBIT_SILU && FAST) {
        const Sigmoid s = sigmoid_relative(g);
        return mul_rn(mul_rn(s.m, add_rn(1.0f, mul_rn(g, s.rest))), s.scale);
    } else if constexpr (ACT == FEWBIT_SILU) {
        const float s = Act<FEWBIT_SIGMOID, FAST>::eval(g, 0.0f, 0.0f);
        return mul_rn(s, add_rn(1.0f, mul_rn(g, sub_rn(1.0f, s))));
    } else {
        const float cdf = mul_rn(0.5f, add_rn(1.0f, erf_precise(mul_rn(g, 0.70710678118654752440f))));
        const float sq = mul_rn(g, g);
        float density;
        if constexpr (FAST) density = __builtin_amdgcn_exp2f(mul_rn(sq, -0.5f * kLog2e));
        else density = expf(mul_rn(sq, -0.5f));
        return add_rn(cdf, mul_rn(g, mul_rn(density, 0.39894228040143267794f)));
    }
}

// ---- the code word of block b of one part: the stores of fewbit_quant.hip ----------------------------------------------------------------------------
template <int BITS> __device__ __forceinline__ void store_word(uint8_t *codes, size_t b, size_t blocks, uint64_t word) {
    if constexpr (BITS == 2) {
        // two lanes' words as one dword from the even lane; the last block of an odd count has no partner inside the part
        const uint32_t mine = static_cast<uint32_t>(word), other = static_cast<uint32_t>(lane_move<kSwapPairs>(static_cast<int>(mine)));
        if ((b & 1) == 0 && b + 1 < blocks) *reinterpret_cast<uint32_t *>(codes + 2 * b) = mine | other << 16;
        else if ((b & 1) == 0 && b < blocks) *reinterpret_cast<uint16_t *>(codes + 2 * b) = static_cast<uint16_t>(mine);
    } else if constexpr (BITS == 4) {
        if (b < blocks) *reinterpret_cast<uint32_t *>(codes + 4 * b) = static_cast<uint32_t>(word);
    } else {
        if (b < blocks) *reinterpret_cast<uint2 *>(codes + 8 * b) = uint2{static_cast<uint32_t>(word), static_cast<uint32_t>(word >> 32)};
    }
}
template <int BITS> __device__ __forceinline__ uint64_t load_word(const uint8_t *codes, size_t b) {
    if constexpr (BITS == 2) return *reinterpret_cast<const uint16_t *>(codes + 2 * b);
    else if constexpr (BITS == 4) return *reinterpret_cast<const uint32_t *>(codes + 4 * b);
    else {
        const uint2 c = *reinterpret_cast<const uint2 *>(codes + 8 * b);
        return c.x | static_cast<uint64_t>(c.y) << 32;
    }
}

// the eight values of a lane -> the parameters of the group its eight lanes hold (every lane of the group gets them)
__device__ __forceinline__ Params group_params(const uint32_t (&x)[kBlock], int have, float levels) {
    int32_t kmin = INT32_MAX, kmax = INT32_MIN;
    uint32_t bad = 0;
#pragma unroll
    for (int e = 0; e < kBlock; ++e) {
        const int32_t k = order_key(x[e]);
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
        bad |= non_finite(x[e]) ? 1u : 0u;
    }
    if (have == 0) kmin = INT32_MAX, kmax = INT32_MIN, bad = 0;
    reduce_step<kSwapPairs>(kmin, kmax, bad);
    reduce_step<kSwapHalves>(kmin, kmax, bad);
    reduce_step<kMirrorEight>(kmin, kmax, bad);
    return params_of(kmin, kmax, bad != 0, levels);
}
template <int BITS, uint32_t DOMAIN>
__device__ __forceinline__ uint64_t code_word(const uint32_t (&x)[kBlock], int have, const Params &p, size_t b, Key key) {
    constexpr uint32_t kLevels = (1u << BITS) - 1u;
    uint32_t w[4];
    block_words<DOMAIN>(b, key, w);
    uint64_t word = 0;
#pragma unroll
    for (int e = 0; e < kBlock; ++e) word |= static_cast<uint64_t>(code_of(float_of_bits(x[e]), p, uniform_of(w, e), kLevels)) << (BITS * e);
    if (have < kBlock) word &= (uint64_t{1} << (BITS * have)) - 1;                                  // the missing elements of the last word are 0
    return word;
}

// BITS = 0: the plain forward, y alone.  state: 8-byte aligned; part g of it (0: gate, 1: up) starts at g * a.part, the parameters of group j at 8 j
// of a part, the code word of block b at 8 groups + BITS b, zero bytes from there to a.part.
template <int DT, int ACT, int BITS, bool VEC>
__global__ __launch_bounds__(kThreads) void glu_forward_kernel(ForwardArgs a) {
    using T = typename Elem<DT>::type;
    constexpr bool kFast = DT != FEWBIT_F32;
    constexpr float kLevels = static_cast<float>((1u << BITS) - 1u);
    const T *gate = static_cast<const T *>(a.gate), *up = static_cast<const T *>(a.up);
    T *y = static_cast<T *>(a.y);
    Key key = a.key;
    if (BITS != 0 && a.device != nullptr) key = *a.device;
    const size_t n = a.n, blocks = (n + kBlock - 1) / kBlock, groups = (n + kGroup - 1) / kGroup, span = static_cast<size_t>(gridDim.x) * kThreads;
    const bool small = (n >> 32) == 0, strided = a.ld_gate != a.width || a.ld_up != a.width;
    // (the bound is a group's, not a block's: the eight lanes of a group leave the loop together, so every lane move below meets its partner)
    for (size_t b = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; b < groups * kLanes; b += span) {
        const size_t i0 = b * kBlock;
        const int have = b >= blocks ? 0 : n - i0 < static_cast<size_t>(kBlock) ? static_cast<int>(n - i0) : kBlock;
        // (rows that follow each other without a gap are the flat tensor: row 0, column i0, and the step to "the next row" is 0 elements long)
        const Where at = strided && have != 0 ? where_of(i0, a.width, small) : Where{0, i0};
        const size_t wrap = strided ? a.width : ~size_t{0};
        T rg[kBlock], ru[kBlock], ry[kBlock];
        load_rows<DT, VEC>(gate, a.ld_gate, wrap, at, have, rg);
        load_rows<DT, VEC>(up, a.ld_up, wrap, at, have, ru);
        uint32_t xg[kBlock], xu[kBlock];
#pragma unroll
        for (int e = 0; e < kBlock; ++e) {
            xg[e] = widen<DT>(rg[e]);
            xu[e] = widen<DT>(ru[e]);
            ry[e] = narrow<DT>(mul_rn(act_of<ACT, kFast>(float_of_bits(xg[e])), float_of_bits(xu[e])));
        }
        store_rows<DT, VEC>(y, 0, ~size_t{0}, Where{0, i0}, have, ry);
        if constexpr (BITS != 0) {
            const Params pg = group_params(xg, have, kLevels), pu = group_params(xu, have, kLevels);
            uint8_t *second = a.state + a.part;
            store_word<BITS>(a.state + 8 * groups, b, blocks, code_word<BITS, kRoundDomain>(xg, have, pg, b, key));
            store_word<BITS>(second + 8 * groups, b, blocks, code_word<BITS, kUpDomain>(xu, have, pu, b, key));
            if ((b & (kLanes - 1)) == 0) {
                *reinterpret_cast<uint2 *>(a.state + 8 * (b / kLanes)) = uint2{bits_of_float(pg.lo), bits_of_float(pg.step)};
                *reinterpret_cast<uint2 *>(second + 8 * (b / kLanes)) = uint2{bits_of_float(pu.lo), bits_of_float(pu.step)};
            }
            if (b + 1 == blocks) {
                // the zero bytes behind the last code word of both parts (none at 8 bits; the used bytes of a part are an even number)
                for (size_t at_byte = 8 * groups + static_cast<size_t>(BITS) * blocks; at_byte < a.part; at_byte += 2) {
                    *reinterpret_cast<uint16_t *>(a.state + at_byte) = 0;
                    *reinterpret_cast<uint16_t *>(second + at_byte) = 0;
                }
            }
        }
    }
}

// PRODUCT: a third output, product[i] = narrow(act(g^) * u^), the forward's own expression on the decodes; gy may then be absent (with both gradients).
// PRODUCT = false is the backward as it was, instruction for instruction (tools/isa_digest.py): the flag is a parameter of the ONE kernel text, not a
// device function both kernels call, and the product's stride is folded in behind the declaration of `gradients_strided` -- either of the other
// two spellings compiles the plain kernels to a few instructions more.
template <int DT, int ACT, int BITS, bool VEC, bool PRODUCT>
__global__ __launch_bounds__(kThreads) void glu_backward_kernel(std::conditional_t<PRODUCT, ProductArgs, BackwardArgs> a) {
    using T = typename Elem<DT>::type;
    constexpr bool kFast = DT != FEWBIT_F32;
    constexpr uint32_t kLevels = (1u << BITS) - 1u;
    const T *gy = static_cast<const T *>(a.gy);
    const size_t n = a.n, blocks = (n + kBlock - 1) / kBlock, groups = (n + kGroup - 1) / kGroup, span = static_cast<size_t>(gridDim.x) * kThreads;
    const uint8_t *second = a.state + a.part;
    const bool want_gate = a.d_gate != nullptr, want_up = a.d_up != nullptr;
    const bool small = (n >> 32) == 0, gradients_strided = (want_gate && a.ld_dgate != a.width) || (want_up && a.ld_dup != a.width);
    bool strided = gradients_strided;
    if constexpr (PRODUCT) strided = strided || (a.product != nullptr && a.ld_product != a.width);
    for (size_t b = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; b < blocks; b += span) {
        const size_t i0 = b * kBlock;
        const int have = n - i0 < static_cast<size_t>(kBlock) ? static_cast<int>(n - i0) : kBlock;
        const uint2 par_g = *reinterpret_cast<const uint2 *>(a.state + 8 * (b / kLanes)), par_u = *reinterpret_cast<const uint2 *>(second + 8 * (b / kLanes));
        const uint64_t word_g = load_word<BITS>(a.state + 8 * groups, b), word_u = load_word<BITS>(second + 8 * groups, b);
        const float lo_g = float_of_bits(par_g.x), step_g = float_of_bits(par_g.y), lo_u = float_of_bits(par_u.x), step_u = float_of_bits(par_u.y);
        // a poisoned group of EITHER input: every output is NaN on its 64 elements
        const bool poisoned = step_g != step_g || step_u != step_u;
        T rgy[kBlock], rdg[kBlock], rdu[kBlock], rpr[kBlock];
        if (PRODUCT && gy == nullptr) {
#pragma unroll
            for (int e = 0; e < kBlock; ++e) rgy[e] = T{0};                                        // (no gradient is wanted: the product alone)
        } else {
            load_rows<DT, VEC>(gy, 0, ~size_t{0}, Where{0, i0}, have, rgy);
        }
#pragma unroll
        for (int e = 0; e < kBlock; ++e) {
            const float g = decode(static_cast<uint32_t>(word_g >> (BITS * e)) & kLevels, lo_g, step_g);
            const float u = decode(static_cast<uint32_t>(word_u >> (BITS * e)) & kLevels, lo_u, step_u);
            const float upstream = float_of_bits(widen<DT>(rgy[e]));
            // (the plain kernels evaluate d_up whether or not it is stored, as they always have; the PRODUCT kernels only where it is wanted)
            if (!PRODUCT || want_up) {
                const float du = mul_rn(upstream, act_of<ACT, kFast>(g));
                rdu[e] = narrow<DT>(poisoned ? float_of_bits(kNaN) : du);
            }
            if (want_gate) {
                const float dg = mul_rn(mul_rn(upstream, u), slope_of<ACT, kFast>(g));
                rdg[e] = narrow<DT>(poisoned ? float_of_bits(kNaN) : dg);
            }
            if constexpr (PRODUCT) {
                if (a.product != nullptr) rpr[e] = narrow<DT>(poisoned ? float_of_bits(kNaN) : mul_rn(act_of<ACT, kFast>(g), u));
            }
        }
        const Where at = strided ? where_of(i0, a.width, small) : Where{0, i0};
        const size_t wrap = strided ? a.width : ~size_t{0};
        if (want_gate) store_rows<DT, VEC>(static_cast<T *>(a.d_gate), a.ld_dgate, wrap, at, have, rdg);
        if (want_up) store_rows<DT, VEC>(static_cast<T *>(a.d_up), a.ld_dup, wrap, at, have, rdu);
        if constexpr (PRODUCT) {
            if (a.product != nullptr) store_rows<DT, VEC>(static_cast<T *>(a.product), a.ld_product, wrap, at, have, rpr);
        }
    }
}

#ifndef FEWBIT_GLU_TU
#define FEWBIT_GLU_TU 0
#endif
constexpr int kUnitDtype = FEWBIT_GLU_TU == 0 ? FEWBIT_F32 : FEWBIT_GLU_TU == 1 ? FEWBIT_F16 : FEWBIT_BF16;

// the kernel of a call, by its record of arguments: the forward (bits = 0: the plain one), the backward or the PRODUCT backward (bits = 0: no kernel)
// (vec before not: the order in which a unit first names its kernels is their order in the device module, fewbit_quant.hip)
template <int DT, class Args> void launch_act(int act, int bits, bool vec, unsigned grid, hipStream_t s, const Args &a) {
    pick<FEWBIT_SILU, FEWBIT_GELU>(act, [&](auto ac) { pick<0, 2, 4, 8>(bits, [&](auto b) { pick<1, 0>(vec, [&](auto v) {
        constexpr int ACT = decltype(ac)::value, BITS = decltype(b)::value;
        constexpr bool VEC = decltype(v)::value != 0;
        if constexpr (std::is_same_v<Args, ForwardArgs>) hipLaunchKernelGGL((glu_forward_kernel<DT, ACT, BITS, VEC>), dim3(grid), dim3(kThreads), 0, s, a);
        else if constexpr (BITS != 0)
            hipLaunchKernelGGL((glu_backward_kernel<DT, ACT, BITS, VEC, std::is_same_v<Args, ProductArgs>>), dim3(grid), dim3(kThreads), 0, s, a);
    }); }); });
}
template <int DT> FEWBIT_HIDDEN void launch_forward(int act, int bits, bool vec, unsigned grid, hipStream_t s, const ForwardArgs &a);
template <int DT> FEWBIT_HIDDEN void launch_backward(int act, int bits, bool vec, unsigned grid, hipStream_t s, const BackwardArgs &a);
template <int DT> FEWBIT_HIDDEN void launch_product(int act, int bits, bool vec, unsigned grid, hipStream_t s, const ProductArgs &a);
template <> void launch_forward<kUnitDtype>(int act, int bits, bool vec, unsigned grid, hipStream_t s, const ForwardArgs &a) {
    launch_act<kUnitDtype>(act, bits, vec, grid, s, a);
}
template <> void launch_backward<kUnitDtype>(int act, int bits, bool vec, unsigned grid, hipStream_t s, const BackwardArgs &a) {
    launch_act<kUnitDtype>(act, bits, vec, grid, s, a);
}

template <> void launch_product<kUnitDtype>(int act, int bits, bool vec, unsigned grid, hipStream_t s, const ProductArgs &a) {
    launch_act<kUnitDtype>(act, bits, vec, grid, s, a);
}

#if FEWBIT_GLU_TU == 0
// bytes of one part: the packed form, filled up to a multiple of 8 (0: no state for these arguments)
inline size_t part_bytes(size_t n, int bits) { return known_bits(bits) && n != 0 && n <= kMaxCount ? (packed_bytes(n, bits) + 7) & ~size_t{7} : 0; }

// what both launches refuse alike: -> 0 to go on with n set, 1 for rows = 0 (FEWBIT_OK, no launch), a negative status otherwise
int shape_of(const char *name, int dtype, int act, size_t rows, size_t width, size_t &n) {
    if (const int rc = check_dtype(name, dtype)) return rc;
    if (act != FEWBIT_SILU && act != FEWBIT_GELU) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: activation %d is neither FEWBIT_SILU nor FEWBIT_GELU", name, act);
    if (rows == 0) return 1;
    if (width == 0 || rows > kMaxCount || width > kMaxCount || rows * width > kMaxCount)
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: %zu x %zu is outside 1 .. 2^36 elements", name, rows, width);
    n = rows * width;
    return 0;
}
#endif

}  // namespace glu
}  // namespace quant
}  // namespace fewbit_hip

#if FEWBIT_GLU_TU == 0
using fewbit_hip::sketch::Key;
namespace glu = fewbit_hip::quant::glu;
namespace quant = fewbit_hip::quant;

// What the two backward entry points share.  `with_product`: fewbit_hipx_glu_backward_product, which alone has a third output, may lack gy where neither
// gradient is wanted, and launches the PRODUCT kernels (the plain entry point keeps its own: they are faster); each words its refusals as it did.
static int backward_call(const char *name, bool with_product, int dtype, int act, const void *gy, const uint8_t *state, size_t rows, size_t width, int bits,
                         void *d_gate, size_t ld_dgate, void *d_up, size_t ld_dup, void *product, size_t ld_product, void *stream) {
    using glu::fail;
    using glu::misaligned;
    size_t n = 0;
    if (const int rc = quant::check_bits(name, bits)) return rc;
    const int shape = glu::shape_of(name, dtype, act, rows, width, n);
    if (shape != 0) return shape < 0 ? shape : FEWBIT_OK;
    if ((d_gate != nullptr && ld_dgate < width) || (d_up != nullptr && ld_dup < width) || (product != nullptr && ld_product < width))
        return with_product ? fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: a row stride (%zu, %zu, %zu) is below the width %zu", name, ld_dgate, ld_dup, ld_product, width)
                            : fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: a row stride (%zu, %zu) is below the width %zu", name, ld_dgate, ld_dup, width);
    if (state == nullptr || (gy == nullptr && !with_product)) return glu::refuse_null(name);
    if (gy == nullptr && (d_gate != nullptr || d_up != nullptr))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: gy is a null pointer and a gradient is wanted (gy may be absent only with d_gate and d_up)", name);
    const size_t item = quant::size_of(dtype);
    if (misaligned(gy, item) || misaligned(d_gate, item) || misaligned(d_up, item) || misaligned(product, item))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: gy, d_gate%s must be aligned to their element size", name, with_product ? ", d_up and product" : " and d_up");
    if (const int rc = glu::check_aligned8(name, "state", state)) return rc;
    if (d_gate == nullptr && d_up == nullptr && product == nullptr) return FEWBIT_OK;
    if (rows == 1) ld_dgate = ld_dup = ld_product = width;
    const auto wide = [&](const void *p, size_t ld) { return p == nullptr || ((ld * item) % 16 == 0 && !misaligned(p, 16)); };
    const bool vec = width % 8 == 0 && !misaligned(gy, 16) && wide(d_gate, ld_dgate) && wide(d_up, ld_dup) && wide(product, ld_product);
    const glu::ProductArgs a{{gy, state, glu::part_bytes(n, bits), width, n, d_gate, d_up, ld_dgate, ld_dup}, product, ld_product};
    const unsigned grid = glu::grid_of((n + quant::kBlock - 1) / quant::kBlock);
    hipStream_t s = static_cast<hipStream_t>(stream);
    glu::pick_dtype(dtype, [&](auto dt) {
        if (with_product) glu::launch_product<decltype(dt)::value>(act, bits, vec, grid, s, a);
        else glu::launch_backward<decltype(dt)::value>(act, bits, vec, grid, s, a);
    });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

extern "C" {

size_t fewbit_hipx_glu_state_bytes(size_t n, int bits) { return 2 * glu::part_bytes(n, bits); }

int fewbit_hipx_glu_state_host(const float *gate_host, const float *up_host, size_t n, int bits, uint64_t seed, uint8_t *out_host) {
    if (const int rc = quant::check_bits("glu_state_host", bits)) return rc;
    if (n == 0) return FEWBIT_OK;
    if (const int rc = glu::check_count("glu_state_host", n)) return rc;
    if (gate_host == nullptr || up_host == nullptr || out_host == nullptr) return glu::refuse_null("glu_state_host");
    const size_t groups = (n + quant::kGroup - 1) / quant::kGroup, part = glu::part_bytes(n, bits), stride = static_cast<size_t>(bits) * quant::kLanes;
    const Key key = fewbit_hip::sketch::key_of(seed);
    std::memset(out_host, 0, 2 * part);
    // (group g starts at block kLanes g of the flat tensor)
    for (size_t g = 0; g < groups; ++g) {
        const size_t first = g * quant::kGroup, count = n - first < static_cast<size_t>(quant::kGroup) ? n - first : quant::kGroup;
        quant::pack_group_host<quant::kRoundDomain>(gate_host + first, count, g * quant::kLanes, key, bits, out_host + 8 * g, out_host + 8 * groups + stride * g);
        quant::pack_group_host<quant::kUpDomain>(up_host + first, count, g * quant::kLanes, key, bits, out_host + part + 8 * g, out_host + part + 8 * groups + stride * g);
    }
    return FEWBIT_OK;
}

int fewbit_hipx_glu_forward(int dtype, int act, const void *gate, size_t ld_gate, const void *up, size_t ld_up, size_t rows, size_t width, int bits, uint64_t seed,
                            const uint64_t *seed_device, void *y, uint8_t *state, size_t state_bytes, void *stream) {
    using glu::fail;
    using glu::misaligned;
    size_t n = 0;
    if (state != nullptr) {
        if (const int rc = quant::check_bits("glu_forward", bits)) return rc;
        if (const int rc = glu::check_seed_word("glu_forward", seed_device)) return rc;
    }
    const int shape = glu::shape_of("glu_forward", dtype, act, rows, width, n);
    if (shape != 0) return shape < 0 ? shape : FEWBIT_OK;
    if (ld_gate < width || ld_up < width) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "glu_forward: a row stride (%zu, %zu) is below the width %zu", ld_gate, ld_up, width);
    if (gate == nullptr || up == nullptr || y == nullptr) return glu::refuse_null("glu_forward");
    const size_t item = quant::size_of(dtype);
    if (misaligned(gate, item) || misaligned(up, item) || misaligned(y, item)) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "glu_forward: gate, up and y must be aligned to their element size");
    const size_t part = state != nullptr ? glu::part_bytes(n, bits) : 0;
    if (const int rc = glu::check_aligned8("glu_forward", "state", state)) return rc;                   // (no state: a null pointer is aligned, and 0 bytes are needed)
    if (const int rc = glu::check_bytes("glu_forward", "state", state_bytes, 2 * part)) return rc;
    // (one row: the stride is never used, and the row is the flat tensor)
    if (rows == 1) ld_gate = ld_up = width;
    const bool vec = width % 8 == 0 && (ld_gate * item) % 16 == 0 && (ld_up * item) % 16 == 0 && !misaligned(gate, 16) && !misaligned(up, 16) && !misaligned(y, 16);
    const glu::ForwardArgs a{gate, up, ld_gate, ld_up, width, n, fewbit_hip::sketch::key_of(seed), reinterpret_cast<const Key *>(seed_device), y, state, part};
    const unsigned grid = glu::grid_of((n + quant::kGroup - 1) / quant::kGroup * quant::kLanes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int kept = state != nullptr ? bits : 0;
    glu::pick_dtype(dtype, [&](auto dt) { glu::launch_forward<decltype(dt)::value>(act, kept, vec, grid, s, a); });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "glu_forward: the launch failed");
}

int fewbit_hipx_glu_backward(int dtype, int act, const void *gy, const uint8_t *state, size_t rows, size_t width, int bits, void *d_gate, size_t ld_dgate, void *d_up,
                             size_t ld_dup, void *stream) {
    return backward_call("glu_backward", false, dtype, act, gy, state, rows, width, bits, d_gate, ld_dgate, d_up, ld_dup, nullptr, 0, stream);
}

int fewbit_hipx_glu_backward_product(int dtype, int act, const void *gy, const uint8_t *state, size_t rows, size_t width, int bits, void *d_gate, size_t ld_dgate,
                                     void *d_up, size_t ld_dup, void *product, size_t ld_product, void *stream) {
    return backward_call("glu_backward_product", true, dtype, act, gy, state, rows, width, bits, d_gate, ld_dgate, d_up, ld_dup, product, ld_product, stream);
}

}  // extern "C"
#endif  // FEWBIT_GLU_TU == 0
