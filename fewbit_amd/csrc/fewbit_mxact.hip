// fewbit_mxact.hip -- the activation between the two linears of a plain MLP, h = act(u), that keeps its input as OCP-MX cells down its columns, and its
// backward, which writes the gradient a second time as fp8 cells and the rebuilt activation as cells only, on gfx950; part of the companion library
// libfewbit_hipx.so (include/fewbit_hipx.h, "The pre-activation as row blocks"):
//
//     mx_act_forward    u (rows x width, own row stride) -> h = act(u) in `dtype` (act in fp32, rounded once) and ONE mx_pack buffer of u            ONE launch
//     mx_act_backward   gh and that buffer -> du = gh * act'(u^) in `dtype`, du as an fp8 'grad' buffer and h^ = act(u^) as an fp4 / fp6 'kept' buffer
//                       only -- the operands of two mx_wgrad calls; h^ itself is never written                                                       ONE launch
//
// Every buffer is bit for bit what mx_pack writes from the tensor in `dtype` with that buffer's seed: the format is fewbit_mxdef.h's (scale_of_amax,
// octet_words, octet_codes, decode, used as they are); silu and gelu (erf) are fewbit_gluact.h's act_of / slope_of as they stand, the tanh form of gelu
// and relu are written here.  What is new is the walk: a column pair in a lane, no LDS, no barrier.
//   wave       a strip of ONE row block (32 rows) x 128 columns; the four waves of a 256-lane workgroup take four neighbouring strips and never meet;
//              the grid walks the strips.
//   lane       l owns columns 2 l, 2 l + 1 of the strip for all 32 rows: one 4-byte access a row at 16 bits, one 8-byte access at fp32 (a wave's row
//              is 256 / 512 contiguous bytes) where the pointer and the row stride allow it and the pair is inside the width, element accesses
//              otherwise -- the same values either way.  Rows and columns outside count as +0.  All 32 row loads are issued before the first is used:
//              loads in flight stand in for occupancy.
//   rounding   what mx::pack_kernel does across lanes happens in the registers of one lane: the amax down a column, the four Philox calls of a column,
//              the codes.  The two columns of a lane run through ONE text (a loop of two rounds that picks the half of each pair), which halves the code.
//   store      a finished cell is one contiguous piece of one lane, 16 B (fp4), 24 B (fp6) or 32 B (fp8), stored by 16- and 8-byte stores; the two cells
//              of a lane are neighbours in the buffer and the cells of a wave are contiguous.  The lane stores its scale bytes itself.
//   backward   the lane loads its two kept cells whole (one 16-byte or three 8-byte loads each, as mx::wgrad_kernel reads them), decodes from registers,
//              walks the 32 rows, stores du as it goes and keeps du and h^ as rounded pairs for the two rounding passes at the end.
//   act        silu, gelu and the tanh form are CALLED (not inlined): 64 evaluations a strip inlined are 80 KB of instructions a kernel, more than the
//              instruction cache of a compute unit pair holds.  relu is inline.
//   poison     a state cell with scale byte 0xFF makes du and h^ NaN on its 32 rows of that column; the cells written from them are poisoned by the
//              ordinary rule of the pack.  No atomics, no workspace: the same arguments give the same bytes.
// Roofline class: memory (forward reads 1 and writes 1 element plus 1 cell; backward reads 1 element plus 1 cell and writes 1 element plus 2 cells).
// Registers: VGPRs of a lane / waves a SIMD, per instantiation (-Rpass-analysis=kernel-resource-usage; the same for all four activations, the count
// of a kernel that calls is that of its calls too); no LDS, no scratch, 106 SGPRs anywhere.  A workgroup is one wave a SIMD, so these are the limit only
// where more workgroups would fit a compute unit.
//                  forward fp4   forward fp6   backward fp4   backward fp6
//     fp32          158 / 3       160 / 3       234 / 2        235 / 2
//     fp16           96 / 5       120 / 4       162 / 3        163 / 3
//     bf16          127 / 4       129 / 3       171 / 2        172 / 2
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "fewbit_hipx.h"
// (fewbit_mxdef.h in front of fewbit_device.h: the definition names kBlock, and fewbit_device.h declares another one in fewbit_hip)
#include "fewbit_mxdef.h"
#include "fewbit_device.h"
#include "fewbit_gluact.h"

#pragma clang fp contract(off)

namespace fewbit_hip {
namespace quant {
namespace mxact {

constexpr int kRows = mx::kCellRows, kOctets = mx::kOctets, kWave = 64, kWaves = 4, kThreads = kWave * kWaves, kStripCols = 2 * kWave;
constexpr size_t kMaxGroups = size_t{1} << 20;            // workgroups; beyond that a wave walks on by the grid's width

struct ForwardArgs {
    const void *u;
    size_t ld_u, rows, width;
    Key key;
    const Key *device;                      // nullptr, or the key in device memory
    void *h;
    size_t ld_h;
    uint8_t *state;                         // may be absent: h alone
    size_t across, count;
    bool vec_u, vec_h;
};
struct BackwardArgs {
    const void *gh;
    size_t ld_gh;
    const uint8_t *state;
    size_t rows, width;
    Key key_du, key_product;
    const Key *device;                      // nullptr, or the two keys in device memory
    void *du;                               // may be absent, and so may either cell buffer: what is absent is not written
    size_t ld_du;
    uint8_t *du_cells, *product_cells;
    size_t across, count;
    bool vec_gh, vec_du;
};

// ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------------------
// The tanh form of gelu, v * 0.5 * (1 + tanh(z)), z = sqrt(2 / pi) (v + 0.044715 v^3).  1 + tanh(z) cancels below z = -1 exactly as 1 + erf does in
// the erf form (fewbit_gluact.h, gelu_relative), and 1 + tanh(z) = 2 sigmoid(2 z) without any cancellation: the value is v * sigmoid(2 z) with
// glu::sigmoid_relative, which holds sigmoid to a few fp32 ulps of ITSELF on the whole line (the rounding of 2 z costs |2 z| 2^-24 of the value:
// 2^-17 at v = -10, where the value is 10^-37).  One operation per step.  v = -inf: -inf * 0 = NaN, as in float64.
constexpr float kTanhA = 0.79788456080286535588f, kTanhC = 0.044715f;
__device__ __forceinline__ float tanh_argument_twice(float v) {
    const float cube = mul_rn(mul_rn(v, v), v);
    return mul_rn(2.0f, mul_rn(kTanhA, add_rn(v, mul_rn(kTanhC, cube))));
}
__device__ __forceinline__ float gelu_tanh_value(float v) {
    const glu::Sigmoid s = glu::sigmoid_relative(tanh_argument_twice(v));
    return mul_rn(mul_rn(v, s.m), s.scale);
}
// its slope: s + v s (1 - s) 2 z', s = sigmoid(2 z), z' = sqrt(2 / pi) (1 + 3 * 0.044715 v^2), as m (1 + v rest 2 z') scale.  Beyond |v| = 32 the slope
// is 1 or -0 in fp32 (s = exp(-2390) there), and v is clamped to that so that v^2 stays finite against rest = 0.  (The clamp swallows a NaN: the
// backward kernel names a poisoned cell itself.)
__device__ __forceinline__ float gelu_tanh_slope(float v) {
    const float c = __builtin_fminf(__builtin_fmaxf(v, -32.0f), 32.0f);
    const glu::Sigmoid s = glu::sigmoid_relative(tanh_argument_twice(c));
    const float twice = mul_rn(2.0f * kTanhA, add_rn(1.0f, mul_rn(3.0f * kTanhC, mul_rn(c, c))));
    return mul_rn(mul_rn(s.m, add_rn(1.0f, mul_rn(mul_rn(c, s.rest), twice))), s.scale);
}

template <int ACT, bool FAST> __device__ __forceinline__ float value_of(float v) {
    if constexpr (ACT == FEWBIT_MXACT_GELU) return glu::act_of<FEWBIT_GELU, FAST>(v);
    else if constexpr (ACT == FEWBIT_MXACT_SILU) return glu::act_of<FEWBIT_SILU, FAST>(v);
    else if constexpr (ACT == FEWBIT_MXACT_GELU_TANH) return gelu_tanh_value(v);
    else return v > 0.0f ? v : (v == v ? 0.0f : v);                    // relu: +0 at and below 0, a NaN stays
}
template <int ACT, bool FAST> __device__ __forceinline__ float slope_at(float v) {
    if constexpr (ACT == FEWBIT_MXACT_GELU) return glu::slope_of<FEWBIT_GELU, FAST>(v);
    else if constexpr (ACT == FEWBIT_MXACT_SILU) return glu::slope_of<FEWBIT_SILU, FAST>(v);
    else if constexpr (ACT == FEWBIT_MXACT_GELU_TANH) return gelu_tanh_slope(v);
    else return v > 0.0f ? 1.0f : 0.0f;                                // relu'(0) = 0
}
// fp32 I/O: the slope in float64, so that du = round(gh * act'(u^)) is ONE rounding of the product.  slope_of<., false> of fewbit_gluact.h is accurate
// relative to the sum of the magnitudes of its terms only (Phi(g) as 0.5 (1 + erf) cancels below g = -2: 340 fp32 ulps of the slope at g = -3, measured),
// which is what fp32 I/O can see.  The value stays act_of<., false>: it has the bytes of the gate and the up of a seed.
template <int ACT> __device__ __forceinline__ double slope_in_double(double v) {
    if constexpr (ACT == FEWBIT_MXACT_GELU) return 0.5 * erfc(v * -0.70710678118654752440) + v * (exp(-0.5 * v * v) * 0.39894228040143267794);
    else if constexpr (ACT == FEWBIT_MXACT_RELU) return v > 0.0 ? 1.0 : 0.0;
    else {
        // silu: g = v, g' = 1; the tanh form: g = 2 z, g' = 2 z'.  s = sigmoid(g): s (1 + v (1 - s) g'), 1 - s as sigmoid(-g)
        const bool tanh_form = ACT == FEWBIT_MXACT_GELU_TANH;
        const double g = tanh_form ? 2.0 * 0.79788456080286535588 * (v + 0.044715 * v * v * v) : v;
        const double by = tanh_form ? 2.0 * 0.79788456080286535588 * (1.0 + 3.0 * 0.044715 * v * v) : 1.0;
        const double s = 1.0 / (1.0 + exp(-g)), rest = 1.0 / (1.0 + exp(g));
        return rest == 0.0 ? s : s * (1.0 + v * rest * by);            // (rest = 0: the slope is 1; v^2 may be inf there)
    }
}
// the calls (header: `act`)
template <bool FAST> struct Both { float value; typename std::conditional<FAST, float, double>::type slope; };
template <int ACT, bool FAST> __device__ __forceinline__ Both<FAST> both_of(float v) {
    if constexpr (FAST) return Both<FAST>{value_of<ACT, FAST>(v), slope_at<ACT, FAST>(v)};
    else return Both<FAST>{value_of<ACT, FAST>(v), slope_in_double<ACT>(static_cast<double>(v))};
}
template <int ACT, bool FAST> __device__ __noinline__ float value_call(float v) { return value_of<ACT, FAST>(v); }
template <int ACT, bool FAST> __device__ __noinline__ Both<FAST> both_call(float v) { return both_of<ACT, FAST>(v); }
template <int ACT, bool FAST> __device__ __forceinline__ float value_in(float v) {
    if constexpr (ACT == FEWBIT_MXACT_RELU) return value_of<ACT, FAST>(v);
    else return value_call<ACT, FAST>(v);
}
template <int ACT, bool FAST> __device__ __forceinline__ Both<FAST> both_in(float v) {
    if constexpr (ACT == FEWBIT_MXACT_RELU) return both_of<ACT, FAST>(v);
    else return both_call<ACT, FAST>(v);
}
// gh * act'(u^), one rounding of the product
__device__ __forceinline__ float times(float upstream, float slope) { return mul_rn(upstream, slope); }
__device__ __forceinline__ float times(float upstream, double slope) { return static_cast<float>(static_cast<double>(upstream) * slope); }

// ---- a lane's part of a strip: 32 rows x 2 columns, a 16-bit pair in one register ------------------------------------------------------------------------
template <int DT> struct Strip {
    using T = typename Elem<DT>::type;
    static constexpr int kWords = DT == FEWBIT_F32 ? 2 : 1;
    uint32_t w[kRows][kWords];
    __device__ __forceinline__ void set(int r, T first, T second) {
        if constexpr (DT == FEWBIT_F32) w[r][0] = first, w[r][1] = second;
        else w[r][0] = static_cast<uint32_t>(first) | static_cast<uint32_t>(second) << 16;
    }
    // (c may be a run-time value: a shift at 16 bits, a select at fp32)
    __device__ __forceinline__ T get(int r, int c) const {
        if constexpr (DT == FEWBIT_F32) return c != 0 ? w[r][1] : w[r][0];
        else return static_cast<T>(w[r][0] >> (16 * c));
    }
};

// whether pair accesses serve a tensor (an absent one: they would)
inline bool paired(const void *p, size_t ld, int dtype) { return !misaligned(p, 2 * size_of(dtype)) && ld % 2 == 0; }

// rows 32 b .. 32 b + 31 of columns col, col + 1 (col even, col < width); all loads are issued before the caller uses one
template <int DT>
__device__ __forceinline__ void load_strip(const typename Elem<DT>::type *src, size_t ld, bool vec, size_t b, size_t col, size_t rows, size_t width, Strip<DT> &s) {
    using T = typename Elem<DT>::type;
    const bool both = col + 1 < width;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const size_t row = kRows * b + r;
        const T *at = src + row * ld + col;
        if (row >= rows) s.set(r, T{0}, T{0});
        else if (vec && both) {
            if constexpr (DT == FEWBIT_F32) {
                const uint2 pair = *reinterpret_cast<const uint2 *>(at);
                s.w[r][0] = pair.x, s.w[r][1] = pair.y;
            } else s.w[r][0] = *reinterpret_cast<const uint32_t *>(at);
        } else s.set(r, at[0], both ? at[1] : T{0});
    }
}
// one row of a pair (row < rows, col < width)
template <int DT>
__device__ __forceinline__ void store_pair(typename Elem<DT>::type *dst, size_t ld, bool vec, size_t row, size_t col, size_t width, const Strip<DT> &s, int r) {
    typename Elem<DT>::type *at = dst + row * ld + col;
    if (vec && col + 1 < width) {
        if constexpr (DT == FEWBIT_F32) *reinterpret_cast<uint2 *>(at) = uint2{s.w[r][0], s.w[r][1]};
        else *reinterpret_cast<uint32_t *>(at) = s.w[r][0];
    } else {
        at[0] = s.get(r, 0);
        if (col + 1 < width) at[1] = s.get(r, 1);
    }
}

// ---- the rounding of mx::pack_kernel on a lane's two columns: amax, scale, four Philox calls and 32 codes a column, all in this lane ---------------------
// `out`: an mx_pack buffer of rows x width (16-byte aligned); col even, col < width
template <int DT, int FMT>
__device__ __forceinline__ void round_strip(const Strip<DT> &s, size_t b, size_t col, size_t rows, size_t width, uint32_t domain, Key key, uint8_t *out) {
    uint8_t *codes = out + mx::codes_offset(rows, width);
#pragma unroll 1
    for (int c = 0; c < 2; ++c) {
        const size_t j = col + c;
        if (j >= width) break;
        uint32_t amax = 0;
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const uint32_t m = widen<DT>(s.get(r, c)) & 0x7fffffffu;
            amax = m > amax ? m : amax;
        }
        const bool bad = amax >= 0x7f800000u;
        const int e = bad ? 128 : mx::scale_of_amax<FMT>(amax);
        uint64_t word[kOctets];
#pragma unroll
        for (int o = 0; o < kOctets; ++o) {
            uint32_t w[4], v[kBlock];
            mx::octet_words(b, j, width, o, domain, key, w);
#pragma unroll
            for (int k = 0; k < kBlock; ++k) v[k] = widen<DT>(s.get(kBlock * o + k, c));
            word[o] = mx::octet_codes<FMT>(v, e, bad, w);
        }
        uint8_t *cell = codes + (b * width + j) * mx::cell_bytes(FMT);
        if constexpr (FMT == 4) {
            *reinterpret_cast<uint4 *>(cell) = uint4{static_cast<uint32_t>(word[0]), static_cast<uint32_t>(word[1]), static_cast<uint32_t>(word[2]),
                                                      static_cast<uint32_t>(word[3])};
        } else if constexpr (FMT == 6) {
            uint64_t *q = reinterpret_cast<uint64_t *>(cell);               // four runs of 48 bits as three words of 64
            q[0] = word[0] | word[1] << 48;
            q[1] = word[1] >> 16 | word[2] << 32;
            q[2] = word[2] >> 32 | word[3] << 16;
        } else {
            uint4 *q = reinterpret_cast<uint4 *>(cell);
            q[0] = uint4{static_cast<uint32_t>(word[0]), static_cast<uint32_t>(word[0] >> 32), static_cast<uint32_t>(word[1]), static_cast<uint32_t>(word[1] >> 32)};
            q[1] = uint4{static_cast<uint32_t>(word[2]), static_cast<uint32_t>(word[2] >> 32), static_cast<uint32_t>(word[3]), static_cast<uint32_t>(word[3] >> 32)};
        }
        out[b * width + j] = static_cast<uint8_t>(e + 127);
    }
}

template <int DT, int ACT, int FMT>
__global__ __launch_bounds__(kThreads) void forward_kernel(ForwardArgs a) {
    using T = typename Elem<DT>::type;
    constexpr bool kFast = DT != FEWBIT_F32;
    const T *u = static_cast<const T *>(a.u);
    T *h = static_cast<T *>(a.h);
    Key key = a.key;
    if (a.device != nullptr && a.state != nullptr) key = a.device[0];
    const size_t rows = a.rows, width = a.width;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (size_t strip = static_cast<size_t>(blockIdx.x) * kWaves + wave; strip < a.count; strip += static_cast<size_t>(gridDim.x) * kWaves) {
        const size_t b = strip / a.across, col = (strip % a.across) * kStripCols + 2 * lane;
        if (col >= width) continue;                        // (no lane waits for another: nothing below crosses lanes)
        Strip<DT> raw, value;
        load_strip<DT>(u, a.ld_u, a.vec_u, b, col, rows, width, raw);
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const size_t row = kRows * b + r;
            if (row >= rows) break;
            const float first = value_in<ACT, kFast>(float_of_bits(widen<DT>(raw.get(r, 0))));
            const float second = value_in<ACT, kFast>(float_of_bits(widen<DT>(raw.get(r, 1))));
            value.set(r, narrow<DT>(first), narrow<DT>(second));
            store_pair<DT>(h, a.ld_h, a.vec_h, row, col, width, value, r);
        }
        if (a.state != nullptr) round_strip<DT, FMT>(raw, b, col, rows, width, mx::kKeptDomain, key, a.state);
    }
}

// the kept cell of column j of block b as dwords (4 at fp4, 6 at fp6), loaded whole
template <int FMT> __device__ __forceinline__ void load_cell(const uint8_t *codes, size_t b, size_t j, size_t width, uint32_t (&cw)[FMT]) {
    const uint8_t *cell = codes + (b * width + j) * mx::cell_bytes(FMT);
    if constexpr (FMT == 4) {
        const uint4 q = *reinterpret_cast<const uint4 *>(cell);
        cw[0] = q.x, cw[1] = q.y, cw[2] = q.z, cw[3] = q.w;
    } else {
        const uint64_t *q = reinterpret_cast<const uint64_t *>(cell);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint64_t two = q[k];
            cw[2 * k] = static_cast<uint32_t>(two), cw[2 * k + 1] = static_cast<uint32_t>(two >> 32);
        }
    }
}
// code r of a cell held as dwords (r a compile-time value once the rows are unrolled)
template <int FMT> __device__ __forceinline__ uint32_t code_in(const uint32_t (&cw)[FMT], int r) {
    const int bit = FMT * r, at = bit / 32, off = bit % 32;
    uint32_t code = cw[at] >> off;
    if (off + FMT > 32) code |= cw[at + 1] << (32 - off);               // (fp6 only, and never in a cell's last dword)
    return code & ((1u << FMT) - 1u);
}

template <int DT, int ACT, int FMT>
__global__ __launch_bounds__(kThreads) void backward_kernel(BackwardArgs a) {
    using T = typename Elem<DT>::type;
    constexpr bool kFast = DT != FEWBIT_F32;
    const T *gh = static_cast<const T *>(a.gh);
    T *du = static_cast<T *>(a.du);
    Key key_du = a.key_du, key_product = a.key_product;
    if (a.device != nullptr) key_du = a.device[0], key_product = a.device[1];
    const size_t rows = a.rows, width = a.width;
    const uint8_t *codes = a.state + mx::codes_offset(rows, width);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (size_t strip = static_cast<size_t>(blockIdx.x) * kWaves + wave; strip < a.count; strip += static_cast<size_t>(gridDim.x) * kWaves) {
        const size_t b = strip / a.across, col = (strip % a.across) * kStripCols + 2 * lane;
        if (col >= width) continue;
        const bool both = col + 1 < width;
        uint32_t first_cell[FMT], second_cell[FMT] = {};
        load_cell<FMT>(codes, b, col, width, first_cell);
        if (both) load_cell<FMT>(codes, b, col + 1, width, second_cell);
        const uint32_t first_scale = a.state[b * width + col], second_scale = both ? a.state[b * width + col + 1] : 127u;
        Strip<DT> upstream, grad, product;
        load_strip<DT>(gh, a.ld_gh, a.vec_gh, b, col, rows, width, upstream);
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const size_t row = kRows * b + r;
            if (row >= rows) {                             // (wave-uniform)
                grad.set(r, T{0}, T{0}), product.set(r, T{0}, T{0});
                continue;
            }
            // a poisoned cell: every output is NaN on its rows of the column (said here: the clamps of the activations swallow a NaN)
            const Both<kFast> p = both_in<ACT, kFast>(mx::decode<FMT>(code_in<FMT>(first_cell, r), first_scale));
            const Both<kFast> q = both_in<ACT, kFast>(mx::decode<FMT>(code_in<FMT>(second_cell, r), second_scale));
            const bool first_bad = first_scale == mx::kPoisonScale, second_bad = second_scale == mx::kPoisonScale;
            const float nan = float_of_bits(kNaN);
            const float d0 = times(float_of_bits(widen<DT>(upstream.get(r, 0))), p.slope), d1 = times(float_of_bits(widen<DT>(upstream.get(r, 1))), q.slope);
            grad.set(r, narrow<DT>(first_bad ? nan : d0), both ? narrow<DT>(second_bad ? nan : d1) : T{0});
            product.set(r, narrow<DT>(first_bad ? nan : p.value), both ? narrow<DT>(second_bad ? nan : q.value) : T{0});
            if (du != nullptr) store_pair<DT>(du, a.ld_du, a.vec_du, row, col, width, grad, r);
        }
        if (a.du_cells != nullptr) round_strip<DT, 8>(grad, b, col, rows, width, mx::kGradDomain, key_du, a.du_cells);
        if (a.product_cells != nullptr) round_strip<DT, FMT>(product, b, col, rows, width, mx::kKeptDomain, key_product, a.product_cells);
    }
}

inline unsigned grid_of(size_t count) {
    const size_t groups = (count + kWaves - 1) / kWaves;
    return static_cast<unsigned>(groups < kMaxGroups ? groups : kMaxGroups);
}

// what both entry points refuse alike, in the order of fewbit_hipx_mx_glu_*; 1: no elements, nothing to do
inline int check_call(const char *name, int dtype, int act, int format, const void *seed_device, size_t rows, size_t width) {
    if (const int rc = check_dtype(name, dtype)) return rc;
    if (act < FEWBIT_MXACT_GELU || act > FEWBIT_MXACT_SILU) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: activation %d is not one of FEWBIT_MXACT_*", name, act);
    if (format != 4 && format != 6) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: format = %d is not 4 (fp4) or 6 (fp6)", name, format);
    if (const int rc = check_seed_word(name, seed_device)) return rc;
    if (rows == 0 || width == 0) return 1;
    if (width > mx::kMaxWidth) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: width = %zu is beyond 2^23", name, width);
    if (rows > kMaxCount / width) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: rows * width = %zu * %zu is beyond 2^36", name, rows, width);
    return FEWBIT_OK;
}
inline int check_aligned16(const char *name, const char *what, const void *p) {
    return !misaligned(p, 16) ? FEWBIT_OK : fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: %s must be 16-byte aligned", name, what);
}

template <class F> void pick_kernel(int dtype, int act, int format, F &&f) {
    pick_dtype(dtype, [&](auto dt) {
        pick<FEWBIT_MXACT_GELU, FEWBIT_MXACT_GELU_TANH, FEWBIT_MXACT_RELU, FEWBIT_MXACT_SILU>(act, [&](auto ac) { pick<4, 6>(format, [&](auto fmt) { f(dt, ac, fmt); }); });
    });
}

}  // namespace mxact
}  // namespace quant
}  // namespace fewbit_hip

using namespace fewbit_hip::quant;
using fewbit_hip::sketch::key_of;

extern "C" {

int fewbit_hipx_mx_act_forward(int dtype, int act, const void *u, size_t ld_u, size_t rows, size_t width, int format, uint64_t seed, const uint64_t *seed_device,
                               void *h, size_t ld_h, uint8_t *state, size_t state_bytes, void *stream) {
    using namespace mxact;
    const char *name = "mx_act_forward";
    if (const int rc = check_call(name, dtype, act, format, seed_device, rows, width)) return rc < 0 ? rc : FEWBIT_OK;
    if (u == nullptr || h == nullptr) return refuse_null(name);
    if (ld_u < width || ld_h < width) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: a row stride ld (%zu, %zu) must be at least width = %zu", name, ld_u, ld_h, width);
    const size_t item = size_of(dtype);
    if (misaligned(u, item) || misaligned(h, item)) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: u and h must be aligned to their element size", name);
    if (const int rc = check_aligned16(name, "state", state)) return rc;
    if (state != nullptr)
        if (const int rc = check_bytes(name, "state", state_bytes, fewbit_hip::mx::bytes_of(rows, width, format))) return rc;
    const size_t across = (width + kStripCols - 1) / kStripCols, count = across * fewbit_hip::mx::blocks_of(rows);
    const ForwardArgs a{u, ld_u, rows, width, key_of(seed), reinterpret_cast<const Key *>(seed_device), h, ld_h, state, across, count, paired(u, ld_u, dtype),
                        paired(h, ld_h, dtype)};
    pick_kernel(dtype, act, format, [&](auto dt, auto ac, auto fmt) {
        hipLaunchKernelGGL((forward_kernel<dt(), ac(), fmt()>), dim3(grid_of(count)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

int fewbit_hipx_mx_act_backward(int dtype, int act, const void *gh, size_t ld_gh, const uint8_t *state, size_t state_bytes, size_t rows, size_t width, int format,
                                uint64_t seed_du, uint64_t seed_product, const uint64_t *seed_device, void *du, size_t ld_du, uint8_t *du_cells,
                                uint8_t *product_cells, void *stream) {
    using namespace mxact;
    const char *name = "mx_act_backward";
    if (const int rc = check_call(name, dtype, act, format, seed_device, rows, width)) return rc < 0 ? rc : FEWBIT_OK;
    if (gh == nullptr || state == nullptr) return refuse_null(name);
    if (ld_gh < width || (du != nullptr && ld_du < width))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: a row stride ld (%zu, %zu) must be at least width = %zu", name, ld_gh, ld_du, width);
    const size_t item = size_of(dtype);
    if (misaligned(gh, item) || misaligned(du, item)) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: gh and du must be aligned to their element size", name);
    if (const int rc = check_aligned16(name, "state", state)) return rc;
    if (const int rc = check_aligned16(name, "du_cells", du_cells)) return rc;
    if (const int rc = check_aligned16(name, "product_cells", product_cells)) return rc;
    if (const int rc = check_bytes(name, "state", state_bytes, fewbit_hip::mx::bytes_of(rows, width, format))) return rc;
    if (du == nullptr && du_cells == nullptr && product_cells == nullptr) return FEWBIT_OK;
    const size_t across = (width + kStripCols - 1) / kStripCols, count = across * fewbit_hip::mx::blocks_of(rows);
    const BackwardArgs a{gh, ld_gh, state, rows, width, key_of(seed_du), key_of(seed_product), reinterpret_cast<const Key *>(seed_device), du, ld_du, du_cells,
                         product_cells, across, count, paired(gh, ld_gh, dtype), paired(du, ld_du, dtype)};
    pick_kernel(dtype, act, format, [&](auto dt, auto ac, auto fmt) {
        hipLaunchKernelGGL((backward_kernel<dt(), ac(), fmt()>), dim3(grid_of(count)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

}  // extern "C"
