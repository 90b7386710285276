// fewbit_gluact.h -- the arithmetic of the gated product act(gate) * up, one element at a time: act and act' in fp32 for silu and gelu (erf), to a few
// fp32 ulps RELATIVE to the value on the whole line for 16-bit I/O.  The ONE text that fewbit_glu.hip (the state in 2, 4 or 8 bits) and
// fewbit_mxglu.hip (the state as MX cells) evaluate; moved here from fewbit_glu.hip as it stood (tools/isa_digest.py: every kernel of that unit has
// the instructions it had, profiles/mxglu_isa_identity.txt).  Include fewbit_device.h and fewbit_quantdef.h first.
#pragma once

namespace fewbit_hip {
namespace quant {
namespace glu {

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

}  // namespace glu
}  // namespace quant
}  // namespace fewbit_hip
