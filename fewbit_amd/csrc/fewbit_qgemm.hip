// fewbit_qgemm.hip -- the weight gradient of a layer that keeps its input in the packed form of a seed, straight from the codes, on gfx950; part of
// the companion library libfewbit_hipx.so (include/fewbit_hipx.h, "The weight gradient from the packed form"):
//
//     out[o][f] = sum_r G[r][o] * op(X^[r][f])        G: rows x out_features (bf16 / fp16, row-major, leading dimension ld_grad)
//                                                     X^: the decode of a quant_pack buffer of rows * in_features elements at `bits` bits
//     op(x) = x rounded once to the dtype of G; for bf16 at 8 bits the two terms head = bf16(x), tail = bf16(x - head), both multiplied onto the
//             SAME fp32 accumulators (kept.decode_in_two_terms: the step of an 8-bit group is about one bf16 ulp)
//
// What it replaces: quant_unpack writing all of X^ to memory (in fp32, then split into two bf16 tensors, at bf16 / 8 bits) and a library GEMM
// reading it back.  Here X^ exists in LDS only: the idea of fewbit_sketch.hip (one MFMA operand is a function evaluated in registers) with
// "S from a seed" replaced by "X^ from its codes".
//
// ---- tiling (ONE plan for every served call; make_plan) ---------------------------------------------------------------------------------------
//   workgroup  8 waves own a tile of BM = 256 out_features x BN = 128 in_features: waves 4 (out) x 2 (in), each 64 x 64 = 2 x 2 blocks of
//              v_mfma_f32_32x32x16_{bf16,f16} -> 64 fp32 accumulators per lane.  The decode of an element is paid once per BM = 256 outputs.
//   K loop     over the rows in stages of BK = 64, double-buffered in LDS (2 x 48 KiB; 2 x 64 KiB with two terms), one barrier per stage: the
//              loads of stage s + 1 go out in front of the MFMAs of stage s and are decoded / transposed into the other buffer behind them.
//   staging    wave w stages octet w (8 rows) of the stage, so every row number -- and with it the clamp and the zeroing of the rows beyond the
//              slice -- is wave-uniform: it lives in scalar registers, and the loads take the scalar-base form.
//     G        a lane takes 8 rows x 4 columns (8 loads of 8 bytes), transposes them with 16 v_perm_b32 and writes 4 pieces of 16 bytes: the
//              image is [octet][chunk], chunk = 32 * (column % 8) + column / 8 -- chunk-major as in the sketch kernel, so a lane's writes and
//              an A fragment (ONE ds_read_b128) are conflict-free.  MFMA block t, row i  <->  column 8 i + t of the tile.
//     X^       a lane takes 8 rows x 2 features: per row ONE load of its two codes (a byte at 2 and 4 bits, two at 8) and ONE of the group's
//              (lo, step); every value is decode() then narrow<>() of fewbit_quantdef.h -- the very functions quant_unpack evaluates -- and the
//              16 values are packed along the rows as they are produced (no permute: every element is computed on its own).  Image:
//              chunk = 32 * (feature % 4) + feature / 4, so the two blocks of a wave hold two NEIGHBOURING features per lane (8-byte stores
//              of the result).  Two terms: a second image of the tails, formed while packing.
//     lanes    lane p takes column group / feature pair 2 (p % 32) + p / 32: the 32 lanes of a half wave then write 32 consecutive chunks.
//   edges      rows at or beyond the slice's end are never loaded: their address is clamped to the slice's last row and BOTH operands are
//              replaced by zeros before they reach LDS (a select, not a product: the bytes behind the buffers may be NaN or unmapped).
//              Columns of the tile outside the matrix are read from column 0: they only feed outputs that are never stored.
//   split K    gridDim.z slices of the rows (multiples of BK) when the tile grid alone cannot fill 256 CUs: slices write fp32 partial sums,
//              a second kernel adds them IN A FIXED ORDER and rounds once.  No atomics: the same inputs give the same bits.  The slice
//              count is capped so that the workspace never exceeds rows * in_features * sizeof(G's dtype), the transient this kernel removes.
// Roofline class: MFMA (bf16 dense peak 2.5 PFLOP/s); flops = 2 * rows * in_features * out_features (twice that with two terms).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fewbit_hipx.h"
#include "fewbit_quantdef.h"

#pragma clang fp contract(off)

namespace fewbit_hip {
namespace qgemm {

using namespace quant;                      // (decode, narrow, widen, sub_rn, the predicates and the refusals of fewbit_unit.h)

constexpr int BM = 256, BN = 128, BK = 64;
constexpr int kWaves = 8, kWgThreads = 64 * kWaves, kSteps = BK / 16, kOctets = BK / 8;
static_assert(kOctets == kWaves, "wave w stages octet w of a stage");
constexpr int kGBytes = kOctets * BM * 16, kXBytes = kOctets * BN * 16;        // one stage of G; one image of X^
constexpr size_t kTargetGroups = 256;       // workgroups the plan tries to reach by slicing the rows (the CUs of an MI355X; the plan does not ask the device)
constexpr size_t kMaxWidth = size_t{1} << 23;

typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

template <int DT> __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
    if constexpr (DT == FEWBIT_BF16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

constexpr bool two_terms(int dtype, int bits) { return dtype == FEWBIT_BF16 && bits == 8; }
constexpr size_t lds_bytes(int dtype, int bits) { return 2 * static_cast<size_t>(kGBytes + (two_terms(dtype, bits) ? 2 : 1) * kXBytes); }

// ---- the plan: a pure function of the extents (cabi_x.quant_wgrad_slices evaluates the same) -----------------------------------------------------
struct Plan { size_t tiles_in, tiles_out, slices, kslice; };

inline bool serves(int dtype, size_t rows, size_t in_features, size_t out_features, int bits) {
    return (dtype == FEWBIT_F16 || dtype == FEWBIT_BF16) && known_bits(bits) && rows >= 1 && in_features >= 1 && in_features <= kMaxWidth &&
           in_features % kGroup == 0 && out_features >= 1 && out_features <= kMaxWidth && out_features % 8 == 0 && rows <= kMaxCount / in_features &&
           out_features * in_features <= kMaxCount;
}

inline Plan make_plan(size_t rows, size_t in_features, size_t out_features) {
    Plan p;
    p.tiles_in = (in_features + BN - 1) / BN;
    p.tiles_out = (out_features + BM - 1) / BM;
    const size_t stages = (rows + BK - 1) / BK, cap = rows / (2 * out_features);      // slices * out * in * 4 <= rows * in * 2
    size_t want = kTargetGroups / (p.tiles_in * p.tiles_out);
    want = want < cap ? want : cap;
    want = want < stages ? want : stages;
    want = want < 65535 ? want : 65535;
    if (want < 2) want = 1;
    const size_t per_slice = (stages + want - 1) / want;
    p.slices = (stages + per_slice - 1) / per_slice;                                   // (no empty slice)
    p.kslice = per_slice * BK;
    return p;
}

inline size_t workspace_of(const Plan &p, size_t in_features, size_t out_features) {
    return p.slices > 1 ? p.slices * out_features * in_features * sizeof(float) : 0;
}

// ---- the kernel -----------------------------------------------------------------------------------------------------------------------------------
// grid: x = tiles along in_features, y = tiles along out_features, z = K slices; `out_`: the result (fp32, or OUT16: the dtype of G), or with
// several slices the workspace, where slice z writes its partial sums (fp32) at z * out_features * in_features
template <int DT, int BITS, bool OUT16>
__global__ __launch_bounds__(kWgThreads) void wgrad_kernel(const uint8_t *__restrict__ grad, size_t ld_bytes, const uint8_t *__restrict__ packed, size_t rows,
                                                           size_t in_features, size_t out_features, size_t kslice, void *__restrict__ out_) {
    constexpr bool TWO = two_terms(DT, BITS);
    constexpr int kStageBytes = kGBytes + (TWO ? 2 : 1) * kXBytes;
    constexpr uint32_t kLevels = (1u << BITS) - 1u;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];                 // 2 x (G, X^ heads [, X^ tails])
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int wm = wave & 3, wn = wave >> 2;                                      // this wave's blocks: rows 2 wm, 2 wm + 1 of G^T x columns 2 wn, 2 wn + 1 of X^
    const size_t n0 = static_cast<size_t>(blockIdx.x) * BN, m0 = static_cast<size_t>(blockIdx.y) * BM;
    const size_t k_begin = static_cast<size_t>(blockIdx.z) * kslice;
    const size_t k_end = k_begin + kslice < rows ? k_begin + kslice : rows;
    if (k_begin >= k_end) return;                                                 // (block-uniform; cannot happen with the host's slicing)
    const size_t nstages = (k_end - k_begin + BK - 1) / BK;

    // staging role of this lane within its wave's octet: columns [4 u, 4 u + 4) of G's tile and features [2 u, 2 u + 2) of X^'s, u = 2 c + h
    const int u = 2 * c + h;
    const size_t gcol = m0 + 4 * u < out_features ? m0 + 4 * u : 0;              // (outside the matrix: column 0, whose products are never stored)
    const size_t xf = n0 + 2 * u < in_features ? n0 + 2 * u : 0;
    const size_t groups_per_row = in_features / kGroup;
    const size_t par_row = 8 * groups_per_row, code_row = in_features / 8 * BITS;
    const uint8_t *codes = packed + par_row * rows;
    const uint32_t goff = static_cast<uint32_t>(gcol * 2), poff = static_cast<uint32_t>(8 * (xf / kGroup)), coff = static_cast<uint32_t>(xf / 2 * BITS / 4);
    const uint32_t nibble = BITS == 2 ? 4u * static_cast<uint32_t>((xf >> 1) & 1) : 0u;      // 2 bits: the byte holds four codes, this lane's pair at bit 0 or 4

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

    u32x2 graw[8], xpar[8];
    uint32_t xcode[8];
    // the loads of stage `st`: row r of the octet is wave-uniform, so a row at or beyond the slice's end is clamped to its last one in scalar registers
    auto fetch = [&](size_t st) __attribute__((always_inline)) {
        const size_t r0 = k_begin + st * BK + 8 * static_cast<size_t>(wave);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const size_t r = r0 + j < k_end ? r0 + j : k_end - 1;
            graw[j] = *reinterpret_cast<const u32x2 *>(grad + r * ld_bytes + goff);
            xpar[j] = *reinterpret_cast<const u32x2 *>(packed + r * par_row + poff);
            if constexpr (BITS == 8) xcode[j] = *reinterpret_cast<const uint16_t *>(codes + r * code_row + coff);
            else xcode[j] = *(codes + r * code_row + coff);
        }
    };
    // registers -> LDS: G transposed, X^ decoded; rows at or beyond the slice's end become zeros of both operands
    auto stage_to_lds = [&](size_t st, uint8_t *buf) __attribute__((always_inline)) {
        const size_t r0 = k_begin + st * BK + 8 * static_cast<size_t>(wave);
        uint16_t head[2][8], tail[2][8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool valid = r0 + j < k_end;                                    // (wave-uniform)
            if (!valid) graw[j] = u32x2{0u, 0u};
            const float lo = float_of_bits(xpar[j].x), step = float_of_bits(xpar[j].y);
            const uint32_t pair = xcode[j] >> nibble;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float v = decode((pair >> (BITS * e)) & kLevels, lo, step);
                const uint16_t hb = narrow<DT>(v);
                head[e][j] = valid ? hb : uint16_t{0};
                if constexpr (TWO) {
                    const uint16_t tb = narrow<DT>(sub_rn(v, float_of_bits(widen<DT>(hb))));
                    tail[e][j] = valid ? tb : uint16_t{0};
                }
            }
        }
        uint8_t *gdst = buf + (static_cast<size_t>(wave) * BM + 128 * h + c) * 16;               // column 4 u + w -> chunk 32 (4 h + w) + c
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int e = w >> 1;
            const uint32_t sel = (w & 1) ? 0x07060302u : 0x05040100u;
            u32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = __builtin_amdgcn_perm(graw[2 * q + 1][e], graw[2 * q][e], sel);
            *reinterpret_cast<u32x4 *>(gdst + 32 * 16 * w) = o;
        }
        uint8_t *xdst = buf + kGBytes + (static_cast<size_t>(wave) * BN + 64 * h + c) * 16;      // feature 2 u + e -> chunk 32 (2 h + e) + c
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            u32x4 o, t;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                o[q] = head[e][2 * q] | static_cast<uint32_t>(head[e][2 * q + 1]) << 16;
                if constexpr (TWO) t[q] = tail[e][2 * q] | static_cast<uint32_t>(tail[e][2 * q + 1]) << 16;
            }
            *reinterpret_cast<u32x4 *>(xdst + 32 * 16 * e) = o;
            if constexpr (TWO) *reinterpret_cast<u32x4 *>(xdst + kXBytes + 32 * 16 * e) = t;
        }
    };

    fetch(0);
    stage_to_lds(0, lds);
    __syncthreads();
    for (size_t s = 0; s < nstages; ++s) {
        const uint8_t *cur = lds + (s & 1) * kStageBytes;
        const bool more = s + 1 < nstages;                                        // (block-uniform)
        if (more) fetch(s + 1);
        // lane (c, h) of step ks reads octet 2 ks + h: 8 consecutive rows of column / feature c of its blocks
        const uint8_t *ga = cur + (static_cast<size_t>(h) * BM + 64 * wm + c) * 16;
        const uint8_t *xb = cur + kGBytes + (static_cast<size_t>(h) * BN + 64 * wn + c) * 16;
#pragma unroll
        for (int ks = 0; ks < kSteps; ++ks) {
            u32x4 a[2], b[2], t[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = *reinterpret_cast<const u32x4 *>(ga + (2 * ks * BM + 32 * i) * 16);
                b[i] = *reinterpret_cast<const u32x4 *>(xb + (2 * ks * BN + 32 * i) * 16);
                if constexpr (TWO) t[i] = *reinterpret_cast<const u32x4 *>(xb + kXBytes + (2 * ks * BN + 32 * i) * 16);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = mfma<DT>(a[i], b[j], acc[i][j]);
                    if constexpr (TWO) acc[i][j] = mfma<DT>(a[i], t[j], acc[i][j]);
                }
        }
        if (more) stage_to_lds(s + 1, lds + ((s + 1) & 1) * kStageBytes);
        __syncthreads();
    }

    // ---- epilogue: accumulator register r of block (i, j) is out_feature 8 ((r & 3) + 8 (r >> 2) + 4 h) + 2 wm + i, in_feature 4 c + 2 wn + j
    const size_t f = n0 + 4 * c + 2 * wn;
    if (f >= in_features) return;                                                 // (in_features is even: the pair is inside or outside)
    const size_t slice_base = static_cast<size_t>(blockIdx.z) * out_features * in_features;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const size_t o = m0 + 8 * ((r & 3) + 8 * (r >> 2) + 4 * h) + 2 * wm + i;
            if (o >= out_features) continue;
            const size_t at = o * in_features + f;
            if constexpr (OUT16) {
                *reinterpret_cast<uint32_t *>(static_cast<uint16_t *>(out_) + at) = narrow<DT>(acc[i][0][r]) | static_cast<uint32_t>(narrow<DT>(acc[i][1][r])) << 16;
            } else {
                *reinterpret_cast<f32x2 *>(static_cast<float *>(out_) + slice_base + at) = f32x2{acc[i][0][r], acc[i][1][r]};
            }
        }
}

// partial sums -> result, four elements per lane: a fixed order (slice 0, 1, 2, ...), one rounding
template <int DT, bool OUT16> __global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ ws, size_t n4, int slices, void *__restrict__ out) {
    const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n4) return;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(ws) + i;
    f32x4 s = src[0];
    for (int z = 1; z < slices; ++z) s += src[static_cast<size_t>(z) * n4];
    if constexpr (OUT16) {
        u32x2 o;
        o.x = narrow<DT>(s.x) | static_cast<uint32_t>(narrow<DT>(s.y)) << 16;
        o.y = narrow<DT>(s.z) | static_cast<uint32_t>(narrow<DT>(s.w)) << 16;
        reinterpret_cast<u32x2 *>(out)[i] = o;
    } else {
        reinterpret_cast<f32x4 *>(out)[i] = s;
    }
}

// f(dtype, bits, out16 as compile-time constants) for the kernels of a call
template <class F> void pick_kernel(int dtype, int bits, bool out16, F &&f) {
    pick<FEWBIT_F16, FEWBIT_BF16>(dtype, [&](auto dt) { pick<2, 4, 8>(bits, [&](auto b) { pick<1, 0>(out16, [&](auto o) { f(dt, b, o); }); }); });
}

}  // namespace qgemm
}  // namespace fewbit_hip

using namespace fewbit_hip;
using namespace fewbit_hip::qgemm;

extern "C" {

size_t fewbit_hipx_quant_wgrad_workspace(int dtype, size_t rows, size_t in_features, size_t out_features, int bits) {
    if (!serves(dtype, rows, in_features, out_features, bits)) return 0;
    return workspace_of(make_plan(rows, in_features, out_features), in_features, out_features);
}

int fewbit_hipx_quant_wgrad(int dtype, const void *grad, size_t ld_grad, const uint8_t *packed, size_t packed_bytes, size_t rows, size_t in_features,
                            size_t out_features, int bits, int out_dtype, void *out, void *workspace, size_t workspace_bytes, void *stream) {
    const char *name = "quant_wgrad";
    if (const int rc = check_dtype(name, dtype)) return rc;
    if (const int rc = check_dtype(name, out_dtype)) return rc;
    if (!known_bits(bits)) return fail(FEWBIT_ERR_UNSUPPORTED, "%s: bits = %d is not 2, 4 or 8", name, bits);
    if (dtype == FEWBIT_F32) return fail(FEWBIT_ERR_UNSUPPORTED, "%s: fp32 gradients are not served (the 16-bit matrix pipe would round them)", name);
    if (out_dtype != FEWBIT_F32 && out_dtype != dtype) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: out_dtype must be F32 or the dtype of grad", name);
    if (rows == 0) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: rows = 0", name);
    if (!serves(dtype, rows, in_features, out_features, bits))
        return fail(FEWBIT_ERR_UNSUPPORTED, "%s: rows = %zu, in_features = %zu, out_features = %zu has no kernel (in_features a multiple of 64, out_features of 8, each up to %zu)",
                    name, rows, in_features, out_features, kMaxWidth);
    if (ld_grad < out_features || ld_grad % 8 != 0) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: ld_grad = %zu must be a multiple of 8 and at least out_features = %zu", name, ld_grad, out_features);
    if (grad == nullptr || packed == nullptr || out == nullptr) return refuse_null(name);
    if (misaligned(grad, 16)) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: grad must be 16-byte aligned", name);
    if (const int rc = check_aligned8(name, "packed", packed)) return rc;
    if (misaligned(out, 16)) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: out must be 16-byte aligned", name);
    if (const int rc = check_bytes(name, "packed", packed_bytes, unit::packed_bytes(rows * in_features, bits))) return rc;
    const Plan plan = make_plan(rows, in_features, out_features);
    const size_t need = workspace_of(plan, in_features, out_features);
    if (need != 0) {
        if (workspace == nullptr) return refuse_null(name);
        if (misaligned(workspace, 16)) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: the workspace must be 16-byte aligned", name);
        if (const int rc = check_bytes(name, "the workspace", workspace_bytes, need)) return rc;
    }
    const bool out16 = out_dtype != FEWBIT_F32, sliced = plan.slices > 1;
    const size_t lds = lds_bytes(dtype, bits);
    const dim3 grid(static_cast<unsigned>(plan.tiles_in), static_cast<unsigned>(plan.tiles_out), static_cast<unsigned>(plan.slices));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = FEWBIT_OK;
    // (a sliced call: the product kernel writes fp32 partial sums into the workspace, the second kernel the result)
    pick_kernel(dtype, bits, out16 && !sliced, [&](auto dt, auto b, auto o) {
        auto kern = wgrad_kernel<dt(), b(), o() != 0>;
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) != hipSuccess) {
            (void)hipGetLastError();
            rc = fail(FEWBIT_ERR_LAUNCH, "%s: cannot reserve %zu bytes of LDS", name, lds);
            return;
        }
        hipLaunchKernelGGL(kern, grid, dim3(kWgThreads), lds, s, static_cast<const uint8_t *>(grad), ld_grad * size_of(dtype), packed, rows, in_features, out_features,
                           plan.kslice, sliced ? workspace : out);
    });
    if (rc != FEWBIT_OK) return rc;
    if (sliced) {
        const size_t n4 = out_features * in_features / 4;
        pick<FEWBIT_F16, FEWBIT_BF16>(dtype, [&](auto dt) {
            pick<1, 0>(out16, [&](auto o) {
                hipLaunchKernelGGL((wgrad_reduce_kernel<dt(), o() != 0>), dim3(static_cast<unsigned>((n4 + 255) / 256)), dim3(256), 0, s, static_cast<const float *>(workspace), n4,
                                   static_cast<int>(plan.slices), out);
            });
        });
    }
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

}  // extern "C"
