// fewbit_norm.hip -- a layer norm that keeps its normalized input in 2, 4 or 8 bits per element for backward, on gfx950; part of the companion
// library libfewbit_hipx.so (include/fewbit_hipx.h, "the normalized rows of a seed"):
//
//     forward   mean, var (two passes over the row in registers), rstd = 1 / sqrt(var + eps), x^ = (x - mean) rstd, y = x^ gamma + beta
//               state = per row and group of 64 (lo, step), then per row the codes of x^ -- the packed form of a seed, rows apart
//     backward  x^q = decode(state), g^ = gy gamma, dx = rstd (g^ - mean(g^) - x^q mean(g^ x^q)), dgamma = sum_r gy x^q, dbeta = sum_r gy
//
// and the RMS norm of the same state ("the un-centred rows"), the same kernels with the kind switched at compile time:
//
//     forward   rstd = 1 / sqrt(mean(x^2) + eps), x^ = x rstd, y = x^ gamma
//     backward  dx = rstd (g^ - x^q mean(g^ x^q)), dgamma = sum_r gy x^q
//
// and both with residual + dropout(x) formed in front ("the sum of a seed in front of the norm"; DropoutAddLayerNorm, DropoutAddRMSNorm), again the same
// kernels with the fusion switched at compile time:
//
//     forward   h = keep ? narrow(x scale + residual) : residual as the blocks are loaded (the mask of the call's seed), then the norm of the rows of h
//     backward  dres = narrow(dx32 + gh), dbranch = keep ? narrow(dres scale) : +0 in place of dx; the sums as before
//
// What QuantizedLayerNorm and QuantizedRMSNorm (fewbit_amd/norm.py) keep: the state and one fp32 rstd per row instead of the input.  lo, step, inv,
// code_of, decode and the poison rule are fewbit_quantdef.h's, the text fewbit_quant.hip evaluates.
//
// The lanes of a row.  A lane holds K blocks of eight elements: block b = k LPR + l for lane l of the LPR lanes of its row, so eight neighbouring
// lanes hold a group (their minimum, maximum and flag meet in three DPP steps) and a row is read once and stays in registers for the
// statistics, for y and for the pack.  A workgroup holds (its lanes) / LPR rows (a tile) and walks the tiles by the grid's width; every
// lane of a workgroup makes every step of every tile -- a lane whose row or block does not exist holds zeros and neutral keys and only its
// loads and stores are switched off -- so each lane move meets an active partner and no barrier sits in divergent control flow.
// The plan, a pure function of (rows, width) (plan_of and backward_plan_of, below, are where the thresholds are decided):
//     width <=   64: LPR =   8  (forward: 32 rows to a workgroup of 256 lanes; backward: 128 rows to one of 1024)
//     width <=  128: LPR =  16            width <= 1024: LPR = 128
//     width <=  512: LPR =  64            width <= 2048: LPR = 256
//     width <= 4096: forward LPR = 256, K = 2; backward LPR =  512, K = 1
//     width <= 8192: forward LPR = 256, K = 4; backward LPR = 1024, K = 1
//   workgroups = min(tiles, 16384) forward, min(tiles, 512) backward (each backward workgroup leaves one row of partial sums, so there are few
//   of them, of 16 waves each).
// A row sum: the lane's own elements in index order, then lanes ^1, ^2, the other quad, the other eight (DPP inside 16 lanes), the four rows of
// 16 of a wave by v_readlane in the order (0 + 16) + (32 + 48), and the waves of a row through LDS in ascending order.  Every lane of a row
// ends with the same bits.
// Backward: ONE launch writes dx and, per workgroup, the sums over its rows of gy x^q and gy for every column into the workspace (the rows of a
// tile are added through LDS in ascending order); a SECOND launch adds the workgroups' partials per column in a fixed order.  No float
// atomics, no flags between workgroups: the same arguments give the same bytes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "fewbit_hipx.h"
#include "fewbit_philox.h"
#include "fewbit_quantdef.h"

#pragma clang fp contract(off)

namespace fewbit_hip {
namespace norm {

using namespace quant;                      // (and with it fewbit_unit.h: fail, the predicates, the mask of a seed, the refusals, pick)

constexpr int kThreads = 256, kBackwardThreads = 1024;       // lanes per workgroup, forward and backward
constexpr size_t kMaxWidth = 8192;
constexpr size_t kMaxGridForward = 16384, kMaxGridBackward = 512;
constexpr int kMirrorSixteen = 0x140;       // row_mirror: by then both halves of the 16 lanes hold their own result

struct Plan { int lpr, k; };                // lanes per row; blocks of eight per lane
// THE thresholds: the narrowest row of lanes that holds the row with one block per lane, up to a whole workgroup; beyond 2048 elements a
// lane takes two or four blocks (32 fp32 registers of row at most)
inline Plan plan_of(size_t width) {
    if (width <= 64) return {8, 1};
    if (width <= 128) return {16, 1};
    if (width <= 512) return {64, 1};
    if (width <= 1024) return {128, 1};
    if (width <= 2048) return {256, 1};
    if (width <= 4096) return {256, 2};
    return {256, 4};
}
// backward: the same thresholds, but beyond 2048 elements a row takes 512 or 1024 lanes of the workgroup's 1024 in place of more blocks per lane
inline Plan backward_plan_of(size_t width) {
    if (width <= 2048) return plan_of(width);
    return {width <= 4096 ? 512 : 1024, 1};
}
inline size_t tiles_of(size_t rows, Plan p, int threads) { const size_t per = threads / p.lpr; return (rows + per - 1) / per; }
inline size_t padded_width(Plan p) { return static_cast<size_t>(p.lpr) * p.k * kBlock; }

inline size_t groups_of(size_t width) { return (width + kGroup - 1) / kGroup; }
inline size_t blocks_of(size_t width) { return (width + kBlock - 1) / kBlock; }
__host__ __device__ inline size_t code_bytes(size_t blocks, int bits) { return (static_cast<size_t>(bits) * blocks + 3) & ~size_t{3}; }
inline bool known_shape(size_t rows, size_t width) { return rows >= 1 && width >= 1 && width <= kMaxWidth && rows <= kMaxCount / width; }
inline size_t state_bytes_of(size_t rows, size_t width, int bits) {
    if (!known_bits(bits) || !known_shape(rows, width)) return 0;
    return rows * (8 * groups_of(width) + code_bytes(blocks_of(width), bits));
}
inline size_t workspace_of(size_t rows, size_t width) {
    if (!known_shape(rows, width)) return 0;
    const Plan p = backward_plan_of(width);
    const size_t tiles = tiles_of(rows, p, kBackwardThreads);
    return (tiles < kMaxGridBackward ? tiles : kMaxGridBackward) * 2 * padded_width(p) * sizeof(float);
}

__device__ __forceinline__ float sqrt_rn(float v) { return __fsqrt_rn(v); }

template <int CTRL> __device__ __forceinline__ float sum_step(float v) {
    return add_rn(v, __builtin_bit_cast(float, lane_move<CTRL>(__builtin_bit_cast(int, v))));
}
__device__ __forceinline__ float lane_value(float v, int lane) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane)); }

// the sum of v over the LPR lanes of a row, the same bits in each of them; `slots`: four floats of LDS of this call's own (LPR >= 128)
template <int LPR> __device__ __forceinline__ float row_sum(float v, float *slots) {
    v = sum_step<kSwapPairs>(v);
    v = sum_step<kSwapHalves>(v);
    v = sum_step<kMirrorEight>(v);
    if constexpr (LPR >= 16) v = sum_step<kMirrorSixteen>(v);
    if constexpr (LPR >= 64) v = add_rn(add_rn(lane_value(v, 0), lane_value(v, 16)), add_rn(lane_value(v, 32), lane_value(v, 48)));
    if constexpr (LPR >= 128) {
        constexpr int kWaves = LPR / 64;
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) slots[wave] = v;
        __syncthreads();
        const int first = wave / kWaves * kWaves;
        v = slots[first];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v = add_rn(v, slots[first + w]);
    }
    return v;
}

// eight elements of a row from element i0 on as fp32; the missing ones (e >= have) are +0
template <int DT> __device__ __forceinline__ void load_block(const typename Elem<DT>::type *p, bool vec, int have, float (&out)[kBlock]) {
    using T = typename Elem<DT>::type;
    T raw[kBlock];
    if (vec && have == kBlock) {
        load8<DT>(p, raw);
    } else {
#pragma unroll
        for (int e = 0; e < kBlock; ++e) raw[e] = e < have ? p[e] : T{0};
    }
#pragma unroll
    for (int e = 0; e < kBlock; ++e) out[e] = float_of_bits(widen<DT>(raw[e]));
}
template <int DT> __device__ __forceinline__ void store_block(typename Elem<DT>::type *p, bool vec, int have, const float (&v)[kBlock]) {
    using T = typename Elem<DT>::type;
    T raw[kBlock];
#pragma unroll
    for (int e = 0; e < kBlock; ++e) raw[e] = narrow<DT>(v[e]);
    if (vec && have == kBlock) {
        store8<DT>(p, raw);
    } else {
#pragma unroll
        for (int e = 0; e < kBlock; ++e)
            if (e < have) p[e] = raw[e];
    }
}
__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- the fusion: residual + dropout(x) in front of the norm, its gradients behind the norm's backward ("the sum of a seed in front of the norm",
// include/fewbit_hipx.h).  The mask is fewbit_dropout.hip's (counter word 3 = 5, one Philox call per block of eight FLAT elements), which a lane's
// block of a row is only where width % 8 == 0: block b of row r is then flat block r * (width / 8) + b, the number the rounding bits take too.
// The kernels gain it as a compile-time switch -- a trailing pack of arguments that is empty (the plain kernels) or one record.
// (kMaskDomain, kOne, mask_bits and scale_of: fewbit_unit.h, the text fewbit_dropout.hip evaluates)
struct NoFusion {};
struct ForwardFusion { const void *residual; void *h_out; uint32_t threshold; float scale; };       // h_out: NULL, or where h is written
// (the backward's `dx` is dres; gh: NULL, or the gradient that arrives at h; dbranch: NULL, or -- with threshold > 0 -- the input's gradient)
struct BackwardFusion { const void *gh; void *dbranch; Key key; const Key *device; uint32_t threshold; float scale; };
__device__ __forceinline__ NoFusion the_fusion() { return {}; }
template <class F> __device__ __forceinline__ const F &the_fusion(const F &f) { return f; }

// the 16 mask bits of the eight elements of flat block q; threshold 0 keeps everything and draws nothing
__device__ __forceinline__ void mask_words(uint64_t q, Key key, uint32_t threshold, uint32_t (&w)[4]) {
    w[0] = w[1] = w[2] = w[3] = ~0u;
    if (threshold != 0) block_words<kMaskDomain>(q, key, w);
}
__device__ __forceinline__ bool kept(const uint32_t (&w)[4], int e, uint32_t threshold) { return mask_bits(w, e) >= threshold; }

// eight elements as they lie in memory; the missing ones are 0
template <int DT> __device__ __forceinline__ void load_raw(const typename Elem<DT>::type *p, bool vec, int have, typename Elem<DT>::type (&raw)[kBlock]) {
    using T = typename Elem<DT>::type;
    if (vec && have == kBlock) {
        load8<DT>(p, raw);
    } else {
#pragma unroll
        for (int e = 0; e < kBlock; ++e) raw[e] = e < have ? p[e] : T{0};
    }
}
template <int DT> __device__ __forceinline__ void store_raw(typename Elem<DT>::type *p, bool vec, int have, const typename Elem<DT>::type (&raw)[kBlock]) {
    if (vec && have == kBlock) {
        store8<DT>(p, raw);
    } else {
#pragma unroll
        for (int e = 0; e < kBlock; ++e)
            if (e < have) p[e] = raw[e];
    }
}
// h = keep ? narrow(widen(x) scale + widen(res)) : res -- `one<DT, true>` of fewbit_dropout.hip: the product and the sum are fp32 values of their
// own (an fp16 operand's conversion, the arithmetic and the rounding must not meet in one v_fma_mix*, which is one step off at the ties).  The two
// texts stay apart: narrow<FEWBIT_F16> has the barrier that `one` places itself, and units 4 and 7 written through `one` change 98 of 98 kernels
// (a plain forward: 483 -> 519 instructions, EXPERIMENTS.md 8.27)
template <int DT> __device__ __forceinline__ typename Elem<DT>::type dropped_sum(typename Elem<DT>::type x, typename Elem<DT>::type res, bool keep, float scale) {
    float v = mul_rn(float_of_bits(widen<DT>(x)), scale);
    if constexpr (DT == FEWBIT_F16) asm("" : "+v"(v));
    v = add_rn(v, float_of_bits(widen<DT>(res)));
    return keep ? narrow<DT>(v) : res;
}
// dbranch = keep ? narrow(widen(dres) scale) : +0 -- `one<DT, false>` of fewbit_dropout.hip
template <int DT> __device__ __forceinline__ typename Elem<DT>::type dropped_gradient(typename Elem<DT>::type dres, bool keep, float scale) {
    const float v = mul_rn(float_of_bits(widen<DT>(dres)), scale);
    return keep ? narrow<DT>(v) : typename Elem<DT>::type{0};
}

// The two norms of this unit are ONE text each for forward and backward, with the kind as a compile-time switch:
//     CENTRED (the layer norm)   two row sums per tile (the row, then the squares of the centred row), beta, dbeta
//     otherwise (the RMS norm)   ONE row sum per tile (the squares of the row as loaded); beta is neither loaded nor added, and backward has no
//                                mean(g^) and no sum of gy
// The slots of row_sum.  row_sum<LPR >= 128> writes slots[wave], meets ONE barrier, then reads its row's slots, so a call may reuse a slot array only
// after another barrier that every wave of the workgroup has met.  With two row sums per tile on two arrays the barrier of the second separates a
// tile's reads of the first array from the next tile's writes to it.  With one row sum per tile that barrier is missing (a fast wave would write
// tile t + 1's value into a slot that a slow wave still reads for tile t), so the array alternates with the parity of the workgroup's own tile
// count: the writes of iteration i + 2 follow the barrier of iteration i + 1, which every wave meets only after its reads of iteration i.
constexpr bool kCentred = true, kUncentred = false;

// BITS = 0: the plain forward that keeps nothing (state is not touched); an un-centred launch passes beta = NULL, which is never read.
// FUSION: nothing (the plain kernel, whose arguments and instructions are what they were before the switch existed), or ONE ForwardFusion: the row
// that is normalized is then h = residual + dropout(x), formed as the blocks are loaded and written to h_out where asked.
template <int DT, int BITS, int LPR, int K, bool CENTRED, class... FUSION>
__global__ __launch_bounds__(kThreads) void forward_kernel(const void *__restrict__ x_, size_t rows, uint32_t width, const void *__restrict__ gamma_,
                                                           const void *__restrict__ beta_, float eps, Key value, const Key *device, void *__restrict__ y_,
                                                           float *__restrict__ rstd_out, uint8_t *__restrict__ state, float *__restrict__ xhat_out,
                                                           FUSION... fusion) {
    using T = typename Elem<DT>::type;
    constexpr bool FUSED = sizeof...(FUSION) != 0;
    [[maybe_unused]] const auto &f = the_fusion(fusion...);
    constexpr int kRowsPerTile = kThreads / LPR;
    constexpr uint32_t kLevels = BITS == 0 ? 1u : (1u << BITS) - 1u;
    __shared__ float slots[2][4];
    const T *x = static_cast<const T *>(x_), *gamma = static_cast<const T *>(gamma_), *beta = static_cast<const T *>(beta_);
    T *y = static_cast<T *>(y_);
    Key key = value;
    if (device != nullptr) key = *device;
    const int sub = threadIdx.x / LPR, l = threadIdx.x % LPR;
    const uint32_t blocks = (width + kBlock - 1) / kBlock, groups = (width + kGroup - 1) / kGroup;
    const size_t tiles = (rows + kRowsPerTile - 1) / kRowsPerTile, stride = BITS == 0 ? 0 : code_bytes(blocks, BITS);
    const float count = static_cast<float>(width);
    const bool vec_gamma = gamma != nullptr && aligned16(gamma), vec_beta = CENTRED && beta != nullptr && aligned16(beta);
    [[maybe_unused]] uint32_t iteration = 0;    // of this workgroup's walk: the parity picks the slots of the one row sum of an un-centred tile
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t r = tile * kRowsPerTile + sub;
        const bool live = r < rows;
        const T *xr = x + r * width;
        T *yr = y + r * width;
        const bool vec_x = aligned16(xr), vec_y = aligned16(yr);
        float v[K][kBlock];
        int have[K];
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t b = static_cast<uint32_t>(k) * LPR + l, i0 = b * kBlock;
            have[k] = !live || b >= blocks ? 0 : width - i0 < static_cast<uint32_t>(kBlock) ? static_cast<int>(width - i0) : kBlock;
            if constexpr (FUSED) {
                const T *rr = static_cast<const T *>(f.residual) + r * width;
                T *hr = static_cast<T *>(f.h_out) + r * width;
                T xs[kBlock], rs[kBlock], hs[kBlock];
                load_raw<DT>(xr + i0, vec_x, have[k], xs);
                load_raw<DT>(rr + i0, aligned16(rr), have[k], rs);
                uint32_t w[4];
                mask_words(static_cast<uint64_t>(r) * blocks + b, key, f.threshold, w);
#pragma unroll
                for (int e = 0; e < kBlock; ++e) {
                    hs[e] = dropped_sum<DT>(xs[e], rs[e], kept(w, e, f.threshold), f.scale);
                    v[k][e] = float_of_bits(widen<DT>(hs[e]));                                      // the norm runs on the ROUNDED sum
                }
                if (f.h_out != nullptr) store_raw<DT>(hr + i0, aligned16(hr), have[k], hs);
            } else {
                load_block<DT>(xr + i0, vec_x, have[k], v[k]);
            }
#pragma unroll
            for (int e = 0; e < kBlock; ++e) s = add_rn(s, CENTRED ? v[k][e] : mul_rn(v[k][e], v[k][e]));  // (a missing element: +0 either way)
        }
        float second;                           // the mean of the squares: of the centred row, or of the row as it is
        if constexpr (CENTRED) {
            const float mean = div_rn(row_sum<LPR>(s, slots[0]), count);
            float ss = 0.0f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
#pragma unroll
                for (int e = 0; e < kBlock; ++e) {
                    v[k][e] = e < have[k] ? sub_rn(v[k][e], mean) : 0.0f;
                    ss = add_rn(ss, mul_rn(v[k][e], v[k][e]));
                }
            }
            second = div_rn(row_sum<LPR>(ss, slots[1]), count);
        } else {
            second = div_rn(row_sum<LPR>(s, slots[iteration & 1]), count);
            ++iteration;
        }
        const float rstd = div_rn(1.0f, sqrt_rn(add_rn(second, eps)));
        if (live && l == 0 && rstd_out != nullptr) rstd_out[r] = rstd;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t b = static_cast<uint32_t>(k) * LPR + l, i0 = b * kBlock;
            float g[kBlock], o[kBlock];
            if (gamma != nullptr) {
                load_block<DT>(gamma + i0, vec_gamma, have[k], g);
            } else {
#pragma unroll
                for (int e = 0; e < kBlock; ++e) g[e] = 1.0f;
            }
            if constexpr (CENTRED) {
                if (beta != nullptr) {
                    load_block<DT>(beta + i0, vec_beta, have[k], o);
                } else {
#pragma unroll
                    for (int e = 0; e < kBlock; ++e) o[e] = 0.0f;
                }
            }
            int32_t kmin = INT32_MAX, kmax = INT32_MIN;
            uint32_t bad = 0;
#pragma unroll
            for (int e = 0; e < kBlock; ++e) {
                v[k][e] = mul_rn(v[k][e], rstd);                                                    // x^
                o[e] = CENTRED ? add_rn(mul_rn(v[k][e], g[e]), o[e]) : mul_rn(v[k][e], g[e]);
                if (e < have[k]) {
                    const uint32_t bits = bits_of_float(v[k][e]);
                    const int32_t key_e = order_key(bits);
                    kmin = key_e < kmin ? key_e : kmin;
                    kmax = key_e > kmax ? key_e : kmax;
                    bad |= non_finite(bits) ? 1u : 0u;
                }
            }
            store_block<DT>(yr + i0, vec_y, have[k], o);
            if (xhat_out != nullptr) {
#pragma unroll
                for (int e = 0; e < kBlock; ++e)
                    if (e < have[k]) xhat_out[r * width + i0 + e] = v[k][e];
            }
            if constexpr (BITS != 0) {
                // the eight lanes of a group: lane ^ 1, lane ^ 2, then the other quad (a lane without elements holds the neutral keys)
                reduce_step<kSwapPairs>(kmin, kmax, bad);
                reduce_step<kSwapHalves>(kmin, kmax, bad);
                reduce_step<kMirrorEight>(kmin, kmax, bad);
                const Params p = params_of(kmin, kmax, bad != 0, static_cast<float>(kLevels));
                uint32_t w[4];
                block_words(static_cast<uint64_t>(r) * blocks + b, key, w);
                uint64_t word = 0;
#pragma unroll
                for (int e = 0; e < kBlock; ++e) word |= static_cast<uint64_t>(code_of(v[k][e], p, uniform_of(w, e), kLevels)) << (BITS * e);
                if (have[k] < kBlock) word &= (uint64_t{1} << (BITS * have[k])) - 1;                // the missing elements of a word are 0
                uint8_t *codes = state + 8 * rows * groups + r * stride;
                if constexpr (BITS == 2) {
                    // two lanes' words as one dword from the even lane; behind the last block of an odd count the row's padding, which is 0
                    const uint32_t mine = static_cast<uint32_t>(word), other = static_cast<uint32_t>(lane_move<kSwapPairs>(static_cast<int>(mine)));
                    if (have[k] > 0 && (b & 1) == 0) *reinterpret_cast<uint32_t *>(codes + 2 * b) = mine | other << 16;
                } else if constexpr (BITS == 4) {
                    if (have[k] > 0) *reinterpret_cast<uint32_t *>(codes + 4 * b) = static_cast<uint32_t>(word);
                } else {
                    if (have[k] > 0) *reinterpret_cast<uint2 *>(codes + 8 * static_cast<size_t>(b)) = uint2{static_cast<uint32_t>(word), static_cast<uint32_t>(word >> 32)};
                }
                if (have[k] > 0 && (l & (kLanes - 1)) == 0)
                    *reinterpret_cast<uint2 *>(state + 8 * (r * groups + b / kLanes)) = uint2{bits_of_float(p.lo), bits_of_float(p.step)};
            }
        }
    }
}

// partials: [workgroup][gy x^q, gy][LPR * 8 columns] fp32, or NULL when neither sum is wanted.  1024 lanes to a workgroup and ONE block per lane
// (a row takes up to 1024 lanes): the column sums of a workgroup's rows stay in 16 registers per lane, and few workgroups -- few rows of
// partials -- still fill the machine.
// Un-centred: ONE row sum per tile (g^ x^q; its slots alternate as in the forward), only the gy x^q accumulators, and only that half of a
// workgroup's partials is written (the layout stays [workgroup][2][columns], which the column sums read with the same stride).
// FUSION: nothing (the plain kernel), or ONE BackwardFusion: what is stored is then dres = narrow(dx32 + gh) (to dx_) and dbranch = the dropout's
// backward of dres, each only where its pointer is given.
template <int DT, int BITS, int LPR, bool CENTRED, class... FUSION>
__global__ __launch_bounds__(kBackwardThreads) void backward_kernel(const void *__restrict__ gy_, const uint8_t *__restrict__ state,
                                                                    const float *__restrict__ rstd_in, const void *__restrict__ gamma_, size_t rows, uint32_t width,
                                                                    void *__restrict__ dx_, float *__restrict__ partials, FUSION... fusion) {
    using T = typename Elem<DT>::type;
    constexpr bool FUSED = sizeof...(FUSION) != 0;
    [[maybe_unused]] const auto &f = the_fusion(fusion...);
    constexpr int kRowsPerTile = kBackwardThreads / LPR;
    constexpr uint32_t kLevels = (1u << BITS) - 1u;
    constexpr int kPadded = LPR * kBlock;
    __shared__ float slots[2][16];
    __shared__ float shared_sums[kRowsPerTile > 1 ? kBackwardThreads * kBlock : 1];
    const T *gy = static_cast<const T *>(gy_), *gamma = static_cast<const T *>(gamma_);
    T *dx = static_cast<T *>(dx_);
    const int sub = threadIdx.x / LPR, l = threadIdx.x % LPR;
    const uint32_t blocks = (width + kBlock - 1) / kBlock, groups = (width + kGroup - 1) / kGroup;
    const size_t tiles = (rows + kRowsPerTile - 1) / kRowsPerTile, stride = code_bytes(blocks, BITS);
    const float count = static_cast<float>(width);
    const uint32_t b = l, i0 = b * kBlock;
    const int have_in_row = b >= blocks ? 0 : width - i0 < static_cast<uint32_t>(kBlock) ? static_cast<int>(width - i0) : kBlock;
    float g[kBlock], acc_gamma[kBlock], acc_beta[kBlock];
    if (gamma != nullptr) {
        load_block<DT>(gamma + i0, aligned16(gamma), have_in_row, g);
    } else {
#pragma unroll
        for (int e = 0; e < kBlock; ++e) g[e] = 1.0f;
    }
#pragma unroll
    for (int e = 0; e < kBlock; ++e) acc_gamma[e] = acc_beta[e] = 0.0f;
    [[maybe_unused]] uint32_t iteration = 0;
    [[maybe_unused]] Key key{};
    if constexpr (FUSED) {
        key = f.key;
        if (f.device != nullptr) key = *f.device;
    }
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t r = tile * kRowsPerTile + sub;
        const bool live = r < rows;
        const int have = live ? have_in_row : 0;
        const T *gr = gy + r * width;
        T *dr = dx + r * width;
        const uint8_t *codes = state + 8 * rows * groups + r * stride;
        float gh[kBlock], xq[kBlock];
        load_block<DT>(gr + i0, aligned16(gr), have, gh);
        uint64_t word = 0;
        uint2 par = uint2{0u, 0u};
        if (have > 0) {
            par = *reinterpret_cast<const uint2 *>(state + 8 * (r * groups + b / kLanes));
            if constexpr (BITS == 2) word = *reinterpret_cast<const uint16_t *>(codes + 2 * b);
            else if constexpr (BITS == 4) word = *reinterpret_cast<const uint32_t *>(codes + 4 * b);
            else {
                const uint2 c = *reinterpret_cast<const uint2 *>(codes + 8 * static_cast<size_t>(b));
                word = c.x | static_cast<uint64_t>(c.y) << 32;
            }
        }
        const float lo = float_of_bits(par.x), step = float_of_bits(par.y);
        [[maybe_unused]] float s1 = 0.0f;
        float s2 = 0.0f;
#pragma unroll
        for (int e = 0; e < kBlock; ++e) {
            xq[e] = e < have ? decode(static_cast<uint32_t>(word >> (BITS * e)) & kLevels, lo, step) : 0.0f;
            if (partials != nullptr && e < have) {
                acc_gamma[e] = add_rn(acc_gamma[e], mul_rn(gh[e], xq[e]));
                if constexpr (CENTRED) acc_beta[e] = add_rn(acc_beta[e], gh[e]);
            }
            gh[e] = mul_rn(gh[e], g[e]);                                                            // g^ (a missing element: +0)
            if constexpr (CENTRED) s1 = add_rn(s1, gh[e]);
            s2 = add_rn(s2, mul_rn(gh[e], xq[e]));
        }
        float m1 = 0.0f, m2;
        if constexpr (CENTRED) {
            m1 = div_rn(row_sum<LPR>(s1, slots[0]), count);
            m2 = div_rn(row_sum<LPR>(s2, slots[1]), count);
        } else {
            m2 = div_rn(row_sum<LPR>(s2, slots[iteration & 1]), count);
            ++iteration;
        }
        bool wanted = dx != nullptr;
        if constexpr (FUSED) wanted = wanted || f.dbranch != nullptr;
        if (wanted) {
            const float rstd = live ? rstd_in[r] : 0.0f;
            float o[kBlock];
#pragma unroll
            for (int e = 0; e < kBlock; ++e) o[e] = mul_rn(rstd, sub_rn(CENTRED ? sub_rn(gh[e], m1) : gh[e], mul_rn(xq[e], m2)));
            if constexpr (FUSED) {
                if (f.gh != nullptr) {
                    const T *ar = static_cast<const T *>(f.gh) + r * width;
                    float arriving[kBlock];
                    load_block<DT>(ar + i0, aligned16(ar), have, arriving);
#pragma unroll
                    for (int e = 0; e < kBlock; ++e) o[e] = add_rn(o[e], arriving[e]);
                }
                T ds[kBlock];
#pragma unroll
                for (int e = 0; e < kBlock; ++e) ds[e] = narrow<DT>(o[e]);                          // dres
                if (dx != nullptr) store_raw<DT>(dr + i0, aligned16(dr), have, ds);
                if (f.dbranch != nullptr) {
                    T *br = static_cast<T *>(f.dbranch) + r * width;
                    uint32_t w[4];
                    mask_words(static_cast<uint64_t>(r) * blocks + b, key, f.threshold, w);
#pragma unroll
                    for (int e = 0; e < kBlock; ++e) ds[e] = dropped_gradient<DT>(ds[e], kept(w, e, f.threshold), f.scale);
                    store_raw<DT>(br + i0, aligned16(br), have, ds);
                }
            } else {
                store_block<DT>(dr + i0, aligned16(dr), have, o);
            }
        }
    }
    if (partials == nullptr) return;                                                                // (the same for every lane of the grid)
    float *mine = partials + static_cast<size_t>(blockIdx.x) * 2 * kPadded;
    constexpr int kSums = CENTRED ? 2 : 1;
    if constexpr (kRowsPerTile == 1) {
        float4 *pg = reinterpret_cast<float4 *>(mine + i0);
        [[maybe_unused]] float4 *pb = reinterpret_cast<float4 *>(mine + kPadded + i0);
        pg[0] = float4{acc_gamma[0], acc_gamma[1], acc_gamma[2], acc_gamma[3]};
        pg[1] = float4{acc_gamma[4], acc_gamma[5], acc_gamma[6], acc_gamma[7]};
        if constexpr (CENTRED) {
            pb[0] = float4{acc_beta[0], acc_beta[1], acc_beta[2], acc_beta[3]};
            pb[1] = float4{acc_beta[4], acc_beta[5], acc_beta[6], acc_beta[7]};
        }
    } else {
        // [row of the tile][column], first for gy x^q, then for gy: the rows of the tile are added in ascending order, a lane per column
#pragma unroll
        for (int which = 0; which < kSums; ++which) {
            if (which == 1) __syncthreads();                                                        // (the first sum has been read)
#pragma unroll
            for (int e = 0; e < kBlock; ++e) shared_sums[sub * kPadded + i0 + e] = which == 0 ? acc_gamma[e] : acc_beta[e];
            __syncthreads();
            for (int c = threadIdx.x; c < kPadded; c += kBackwardThreads) {
                float t = shared_sums[c];
                for (int j = 1; j < kRowsPerTile; ++j) t = add_rn(t, shared_sums[j * kPadded + c]);
                mine[which * kPadded + c] = t;
            }
        }
    }
}

#if !defined(FEWBIT_NORM_TU) || FEWBIT_NORM_TU == 0
// dgamma[c] / dbeta[c] = the sum of the workgroups' partials of column c.  A workgroup of 16 waves takes 64 columns of one of the two sums: wave
// w adds the partials w, w + 16, w + 32, .. as four interleaved running sums (every fourth of them each), combined as (0 + 1) + (2 + 3), and
// the 16 waves' results are added in ascending order.
__global__ __launch_bounds__(kBackwardThreads) void column_sums_kernel(const float *__restrict__ partials, uint32_t parts, uint32_t padded, uint32_t width,
                                                                       float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ float waves[16][64];
    const uint32_t chunks = (width + 63) / 64, which = blockIdx.x / chunks, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t c = (blockIdx.x % chunks) * 64 + lane;
    float *out = which == 0 ? dgamma : dbeta;
    if (out == nullptr) return;                                                                     // (the same for every lane of the workgroup)
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (c < width) {
        const float *p = partials + static_cast<size_t>(which) * padded + c;
        for (uint32_t i = wave; i < parts; i += 64) {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (i + 16 * j < parts) a[j] = add_rn(a[j], p[static_cast<size_t>(i + 16 * j) * 2 * padded]);
        }
    }
    waves[wave][lane] = add_rn(add_rn(a[0], a[1]), add_rn(a[2], a[3]));
    __syncthreads();
    if (wave == 0 && c < width) {
        float t = waves[0][lane];
#pragma unroll
        for (int w = 1; w < 16; ++w) t = add_rn(t, waves[w][lane]);
        out[c] = t;
    }
}

#endif

struct ForwardArgs {
    const void *x; size_t rows; uint32_t width; const void *gamma, *beta; float eps; Key key; const Key *device; void *y; float *rstd; uint8_t *state; float *xhat;
    ForwardFusion add;                          // read by the fused units only
};
struct BackwardArgs {
    const void *gy; const uint8_t *state; const float *rstd; const void *gamma; size_t rows; uint32_t width; void *dx; float *partials;
    BackwardFusion add;                         // read by the fused units only; dx is dres there
};

// one unit per dtype, kind and fusion, compiled in parallel and linked into one library: -DFEWBIT_NORM_TU=0 / 1 / 2 the layer norm (fp32 with the C
// entry points of every norm and the column sums, fp16, bf16), 3 / 4 / 5 the RMS norm in the same order of dtypes, 6 .. 11 the same six with
// residual + dropout(x) in front (the kernels with a fusion record and nothing else)
#ifndef FEWBIT_NORM_TU
#define FEWBIT_NORM_TU 0
#endif
constexpr int kUnitDtype = FEWBIT_NORM_TU % 3 == 0 ? FEWBIT_F32 : FEWBIT_NORM_TU % 3 == 1 ? FEWBIT_F16 : FEWBIT_BF16;
constexpr bool kUnitCentred = FEWBIT_NORM_TU % 6 < 3, kUnitFused = FEWBIT_NORM_TU >= 6;

// (FUSED is part of every launcher's name: the units are linked into one library, where two instantiations of one name would be ONE function)
template <int DT, int BITS, int LPR, int K, bool CENTRED, bool FUSED> void launch(unsigned grid, hipStream_t s, const ForwardArgs &a) {
    if constexpr (FUSED)
        hipLaunchKernelGGL((forward_kernel<DT, BITS, LPR, K, CENTRED, ForwardFusion>), dim3(grid), dim3(kThreads), 0, s, a.x, a.rows, a.width, a.gamma, a.beta, a.eps,
                           a.key, a.device, a.y, a.rstd, a.state, a.xhat, a.add);
    else
        hipLaunchKernelGGL((forward_kernel<DT, BITS, LPR, K, CENTRED>), dim3(grid), dim3(kThreads), 0, s, a.x, a.rows, a.width, a.gamma, a.beta, a.eps, a.key, a.device,
                           a.y, a.rstd, a.state, a.xhat);
}
template <int DT, int BITS, int LPR, bool CENTRED, bool FUSED> void launch_backward_lanes(unsigned grid, hipStream_t s, const BackwardArgs &a) {
    if constexpr (BITS != 0 && FUSED)
        hipLaunchKernelGGL((backward_kernel<DT, BITS, LPR, CENTRED, BackwardFusion>), dim3(grid), dim3(kBackwardThreads), 0, s, a.gy, a.state, a.rstd, a.gamma, a.rows,
                           a.width, a.dx, a.partials, a.add);
    else if constexpr (BITS != 0)
        hipLaunchKernelGGL((backward_kernel<DT, BITS, LPR, CENTRED>), dim3(grid), dim3(kBackwardThreads), 0, s, a.gy, a.state, a.rstd, a.gamma, a.rows, a.width, a.dx,
                           a.partials);
}
// the kernel of a plan (plan_of, backward_plan_of: a lane has more than one block only where a row takes a forward workgroup's 256 lanes)
template <int DT, bool CENTRED, bool FUSED> void launch_bits(int bits, Plan p, unsigned grid, hipStream_t s, const ForwardArgs &a) {
    pick<0, 2, 4, 8>(bits, [&](auto b) { pick<8, 16, 64, 128, 256>(p.lpr, [&](auto lpr) { pick<1, 2, 4>(p.k, [&](auto k) {
        constexpr int LPR = decltype(lpr)::value, K = decltype(k)::value;
        if constexpr (LPR == 256 || K == 1) launch<DT, decltype(b)::value, LPR, K, CENTRED, FUSED>(grid, s, a);
    }); }); });
}
template <int DT, bool CENTRED, bool FUSED> void launch_bits(int bits, Plan p, unsigned grid, hipStream_t s, const BackwardArgs &a) {
    pick<0, 2, 4, 8>(bits, [&](auto b) { pick<8, 16, 64, 128, 256, 512, 1024>(p.lpr, [&](auto lpr) {
        launch_backward_lanes<DT, decltype(b)::value, decltype(lpr)::value, CENTRED, FUSED>(grid, s, a);
    }); });
}
template <int DT, bool CENTRED, bool FUSED> FEWBIT_HIDDEN void launch_forward(int bits, Plan p, unsigned grid, hipStream_t s, const ForwardArgs &a);
template <int DT, bool CENTRED, bool FUSED> FEWBIT_HIDDEN void launch_backward(int bits, Plan p, unsigned grid, hipStream_t s, const BackwardArgs &a);
template <> void launch_forward<kUnitDtype, kUnitCentred, kUnitFused>(int bits, Plan p, unsigned grid, hipStream_t s, const ForwardArgs &a) {
    launch_bits<kUnitDtype, kUnitCentred, kUnitFused>(bits, p, grid, s, a);
}
template <> void launch_backward<kUnitDtype, kUnitCentred, kUnitFused>(int bits, Plan p, unsigned grid, hipStream_t s, const BackwardArgs &a) {
    launch_bits<kUnitDtype, kUnitCentred, kUnitFused>(bits, p, grid, s, a);
}

#if FEWBIT_NORM_TU == 0
template <bool CENTRED, bool FUSED> void launch_dtype(int dtype, int bits, Plan p, unsigned grid, hipStream_t s, const ForwardArgs &a) {
    pick_dtype(dtype, [&](auto dt) { launch_forward<decltype(dt)::value, CENTRED, FUSED>(bits, p, grid, s, a); });
}
template <bool CENTRED, bool FUSED> void launch_dtype(int dtype, int bits, Plan p, unsigned grid, hipStream_t s, const BackwardArgs &a) {
    pick_dtype(dtype, [&](auto dt) { launch_backward<decltype(dt)::value, CENTRED, FUSED>(bits, p, grid, s, a); });
}

// the refusals of a shape that every entry point shares, host and device; 1: nothing to do
int check_extent(const char *name, size_t rows, size_t width) {
    if (width == 0 || width > kMaxWidth) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: width = %zu is outside 1 .. %zu", name, width, kMaxWidth);
    if (rows == 0) return 1;
    if (rows > kMaxCount / width) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: rows * width = %zu * %zu is beyond 2^36", name, rows, width);
    return FEWBIT_OK;
}
// the device entry points: the dtype first
int check_shape(const char *name, int dtype, size_t rows, size_t width) {
    if (const int rc = check_dtype(name, dtype)) return rc;
    return check_extent(name, rows, width);
}
// the host entry points: the bits first, the pointers last
int check_host(const char *name, size_t rows, size_t width, int bits, const void *from, const void *to) {
    if (const int rc = check_bits(name, bits)) return rc;
    const int shape = check_extent(name, rows, width);
    if (shape != FEWBIT_OK) return shape;
    return from == nullptr || to == nullptr ? refuse_null(name) : FEWBIT_OK;
}

// what the fused entry points refuse on top, forward and backward: a threshold that drops everything or more, and a mask on rows whose blocks of
// eight are not the flat tensor's
int check_threshold(const char *name, uint32_t threshold, size_t width) {
    if (threshold >= kOne) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: threshold = %u is outside 0 .. 65535", name, threshold);
    if (threshold != 0 && width % kBlock != 0)
        return fail(FEWBIT_ERR_UNSUPPORTED, "%s: a mask (threshold = %u) needs a width that is a multiple of 8, not %zu", name, threshold, width);
    return FEWBIT_OK;
}

// the forward entry point of either norm: the refusals, the plan, ONE launch (the RMS norm: beta = NULL); `add`: the fused call's residual, h_out and
// threshold (its scale is filled in here), NULL for the plain one
template <bool CENTRED>
int forward_call(const char *name, int dtype, const void *x, size_t rows, size_t width, const void *gamma, const void *beta, double eps, int bits, uint64_t seed,
                 const uint64_t *seed_device, void *y, float *rstd, uint8_t *state, size_t state_bytes, float *xhat_out, void *stream,
                 const ForwardFusion *add = nullptr) {
    const int shape = check_shape(name, dtype, rows, width);
    if (shape < 0) return shape;
    if (add != nullptr) {
        const int refused = check_threshold(name, add->threshold, width);
        if (refused != FEWBIT_OK) return refused;
    }
    if (state != nullptr)
        if (const int rc = check_bits(name, bits)) return rc;
    if (!(eps >= 0.0) || !std::isfinite(eps)) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: eps = %g is not a finite number >= 0", name, eps);
    if (const int rc = check_seed_word(name, seed_device)) return rc;
    if (shape == 1) return FEWBIT_OK;
    if (x == nullptr || y == nullptr) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: null pointer (x or y)", name);
    if (add != nullptr && add->residual == nullptr) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: null pointer (residual)", name);
    if (state != nullptr && rstd == nullptr) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: null pointer (rstd goes with the state)", name);
    const size_t size = size_of(dtype);
    if (misaligned(x, size) || misaligned(y, size) || misaligned(gamma, size) || misaligned(beta, size))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: %s must be aligned to their element size", name, CENTRED ? "x, y, gamma and beta" : "x, y and gamma");
    if (add != nullptr && (misaligned(add->residual, size) || misaligned(add->h_out, size)))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: residual and h_out must be aligned to their element size", name);
    if (misaligned(rstd, 4) || misaligned(xhat_out, 4)) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: rstd and xhat_out must be 4-byte aligned", name);
    if (const int rc = check_aligned8(name, "state", state)) return rc;
    if (state != nullptr)
        if (const int rc = check_bytes(name, "state", state_bytes, state_bytes_of(rows, width, bits))) return rc;
    const Plan p = plan_of(width);
    const size_t tiles = tiles_of(rows, p, kThreads);
    const unsigned grid = static_cast<unsigned>(tiles < kMaxGridForward ? tiles : kMaxGridForward);
    ForwardArgs a{x, rows, static_cast<uint32_t>(width), gamma, beta, static_cast<float>(eps), sketch::key_of(seed), reinterpret_cast<const Key *>(seed_device),
                  y, rstd, state, xhat_out, {}};
    if (add != nullptr) {
        a.add = ForwardFusion{add->residual, add->h_out, add->threshold, scale_of(add->threshold)};
        launch_dtype<CENTRED, true>(dtype, state != nullptr ? bits : 0, p, grid, static_cast<hipStream_t>(stream), a);
    } else {
        launch_dtype<CENTRED, false>(dtype, state != nullptr ? bits : 0, p, grid, static_cast<hipStream_t>(stream), a);
    }
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

// the backward entry point of either norm: the refusals, the plan, the launch of dx and the partials, then the column sums (the RMS norm: dbeta =
// NULL, and the column sums are launched for dgamma alone)
// `add`: the fused call's gh, dbranch, seed and threshold (dx is its dres; its scale is filled in here), NULL for the plain one
template <bool CENTRED>
int backward_call(const char *name, int dtype, const void *gy, const uint8_t *state, const float *rstd, const void *gamma, size_t rows, size_t width, int bits,
                  void *dx, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, void *stream, const BackwardFusion *add = nullptr) {
    const int shape = check_shape(name, dtype, rows, width);
    if (shape < 0) return shape;
    if (add != nullptr) {
        const int refused = check_threshold(name, add->threshold, width);
        if (refused != FEWBIT_OK) return refused;
        if (add->dbranch != nullptr && add->threshold == 0)
            return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: with threshold = 0 dbranch is dres: pass dbranch = NULL", name);
        if (const int rc = check_seed_word(name, add->device)) return rc;
    }
    void *const dbranch = add != nullptr ? add->dbranch : nullptr;
    if (const int rc = check_bits(name, bits)) return rc;
    if (shape == 1) return FEWBIT_OK;
    if (gy == nullptr || state == nullptr) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: null pointer (gy or state)", name);
    if ((dx != nullptr || dbranch != nullptr) && rstd == nullptr)
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: null pointer (%s rstd)", name, add != nullptr ? "dres and dbranch need" : "dx needs");
    const size_t size = size_of(dtype);
    if (misaligned(gy, size) || misaligned(dx, size) || misaligned(gamma, size))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: gy, %s and gamma must be aligned to their element size", name, add != nullptr ? "dres" : "dx");
    if (add != nullptr && (misaligned(add->gh, size) || misaligned(dbranch, size)))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: gh and dbranch must be aligned to their element size", name);
    if (misaligned(rstd, 4) || misaligned(dgamma, 4) || misaligned(dbeta, 4))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: %s must be 4-byte aligned", name, CENTRED ? "rstd, dgamma and dbeta" : "rstd and dgamma");
    if (const int rc = check_aligned8(name, "state", state)) return rc;
    const bool sums = dgamma != nullptr || dbeta != nullptr;
    if (dx == nullptr && dbranch == nullptr && !sums) return FEWBIT_OK;
    if (sums && (workspace == nullptr || misaligned(workspace, 16))) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: the workspace must be 16-byte aligned", name);
    if (sums)
        if (const int rc = check_bytes(name, "the workspace", workspace_bytes, workspace_of(rows, width))) return rc;
    const Plan p = backward_plan_of(width);
    const size_t tiles = tiles_of(rows, p, kBackwardThreads);
    const unsigned grid = static_cast<unsigned>(tiles < kMaxGridBackward ? tiles : kMaxGridBackward);
    hipStream_t s = static_cast<hipStream_t>(stream);
    BackwardArgs a{gy, state, rstd, gamma, rows, static_cast<uint32_t>(width), dx, sums ? static_cast<float *>(workspace) : nullptr, {}};
    if (add != nullptr) {
        a.add = *add;
        a.add.scale = scale_of(add->threshold);
        launch_dtype<CENTRED, true>(dtype, bits, p, grid, s, a);
    } else {
        launch_dtype<CENTRED, false>(dtype, bits, p, grid, s, a);
    }
    if (hipGetLastError() != hipSuccess) return fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
    if (sums) {
        // a workgroup per 64 columns of each sum; the un-centred backward wrote only the first half of the partials, and only that is read
        const unsigned chunks = (CENTRED ? 2 : 1) * static_cast<unsigned>((width + 63) / 64);
        hipLaunchKernelGGL(column_sums_kernel, dim3(chunks), dim3(kBackwardThreads), 0, s, static_cast<const float *>(workspace), grid,
                           static_cast<uint32_t>(padded_width(p)), static_cast<uint32_t>(width), dgamma, dbeta);
        if (hipGetLastError() != hipSuccess) return fail(FEWBIT_ERR_LAUNCH, "%s: the launch of the column sums failed", name);
    }
    return FEWBIT_OK;
}

#endif  // FEWBIT_NORM_TU == 0

}  // namespace norm
}  // namespace fewbit_hip

#if FEWBIT_NORM_TU == 0
using namespace fewbit_hip;
using namespace fewbit_hip::norm;

extern "C" {

size_t fewbit_hipx_norm_state_bytes(size_t rows, size_t width, int bits) { return state_bytes_of(rows, width, bits); }

size_t fewbit_hipx_norm_workspace(size_t rows, size_t width) { return workspace_of(rows, width); }

int fewbit_hipx_norm_state_host(const float *xhat_host, size_t rows, size_t width, int bits, uint64_t seed, uint8_t *out_host) {
    const int refused = check_host("norm_state_host", rows, width, bits, xhat_host, out_host);
    if (refused != FEWBIT_OK) return refused < 0 ? refused : FEWBIT_OK;
    const size_t groups = groups_of(width), blocks = blocks_of(width), stride = code_bytes(blocks, bits);
    const Key key = sketch::key_of(seed);
    // (group g of row r starts at block kLanes g of the row's `blocks`; the padding behind a row's code bytes is 0)
    for (size_t r = 0; r < rows; ++r) {
        uint8_t *codes = out_host + 8 * rows * groups + r * stride;
        std::memset(codes, 0, stride);
        for (size_t g = 0; g < groups; ++g) {
            const size_t first = g * kGroup, count = width - first < static_cast<size_t>(kGroup) ? width - first : kGroup;
            pack_group_host(xhat_host + r * width + first, count, static_cast<uint64_t>(r) * blocks + g * kLanes, key, bits, out_host + 8 * (r * groups + g),
                            codes + static_cast<size_t>(bits) * kLanes * g);
        }
    }
    return FEWBIT_OK;
}

int fewbit_hipx_norm_state_unpack_host(const uint8_t *state_host, size_t rows, size_t width, int bits, float *out_host) {
    const int refused = check_host("norm_state_unpack_host", rows, width, bits, state_host, out_host);
    if (refused != FEWBIT_OK) return refused < 0 ? refused : FEWBIT_OK;
    const size_t groups = groups_of(width), stride = code_bytes(blocks_of(width), bits);
    for (size_t r = 0; r < rows; ++r) {
        const uint8_t *params = state_host + 8 * r * groups, *codes = state_host + 8 * rows * groups + r * stride;
        for (size_t i = 0; i < width; ++i) out_host[r * width + i] = decode_host(params, codes, i, bits);
    }
    return FEWBIT_OK;
}

int fewbit_hipx_layer_norm_forward(int dtype, const void *x, size_t rows, size_t width, const void *gamma, const void *beta, double eps, int bits, uint64_t seed,
                                   const uint64_t *seed_device, void *y, float *rstd, uint8_t *state, size_t state_bytes, float *xhat_out, void *stream) {
    return forward_call<kCentred>("layer_norm_forward", dtype, x, rows, width, gamma, beta, eps, bits, seed, seed_device, y, rstd, state, state_bytes, xhat_out, stream);
}

int fewbit_hipx_layer_norm_backward(int dtype, const void *gy, const uint8_t *state, const float *rstd, const void *gamma, size_t rows, size_t width, int bits,
                                    void *dx, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, void *stream) {
    return backward_call<kCentred>("layer_norm_backward", dtype, gy, state, rstd, gamma, rows, width, bits, dx, dgamma, dbeta, workspace, workspace_bytes, stream);
}

int fewbit_hipx_rms_norm_forward(int dtype, const void *x, size_t rows, size_t width, const void *gamma, double eps, int bits, uint64_t seed,
                                 const uint64_t *seed_device, void *y, float *rstd, uint8_t *state, size_t state_bytes, float *xhat_out, void *stream) {
    return forward_call<kUncentred>("rms_norm_forward", dtype, x, rows, width, gamma, nullptr, eps, bits, seed, seed_device, y, rstd, state, state_bytes, xhat_out,
                                    stream);
}

int fewbit_hipx_rms_norm_backward(int dtype, const void *gy, const uint8_t *state, const float *rstd, const void *gamma, size_t rows, size_t width, int bits,
                                  void *dx, float *dgamma, void *workspace, size_t workspace_bytes, void *stream) {
    return backward_call<kUncentred>("rms_norm_backward", dtype, gy, state, rstd, gamma, rows, width, bits, dx, dgamma, nullptr, workspace, workspace_bytes, stream);
}

// residual + dropout(x) in front of either norm: the plain entry points' arguments plus the residual, the threshold and where h goes; backward gives
// the gradient of the residual (dres, with the gradient arriving at h added) and of the input (dbranch) in place of dx
int fewbit_hipx_add_layer_norm_forward(int dtype, const void *x, const void *residual, size_t rows, size_t width, const void *gamma, const void *beta, double eps,
                                       int bits, uint64_t seed, const uint64_t *seed_device, uint32_t threshold, void *y, void *h_out, float *rstd, uint8_t *state,
                                       size_t state_bytes, float *xhat_out, void *stream) {
    const ForwardFusion add{residual, h_out, threshold, 0.0f};
    return forward_call<kCentred>("add_layer_norm_forward", dtype, x, rows, width, gamma, beta, eps, bits, seed, seed_device, y, rstd, state, state_bytes, xhat_out,
                                  stream, &add);
}

int fewbit_hipx_add_layer_norm_backward(int dtype, const void *gy, const void *gh, const uint8_t *state, const float *rstd, const void *gamma, size_t rows,
                                        size_t width, int bits, uint64_t seed, const uint64_t *seed_device, uint32_t threshold, void *dres, void *dbranch,
                                        float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, void *stream) {
    const BackwardFusion add{gh, dbranch, sketch::key_of(seed), reinterpret_cast<const Key *>(seed_device), threshold, 0.0f};
    return backward_call<kCentred>("add_layer_norm_backward", dtype, gy, state, rstd, gamma, rows, width, bits, dres, dgamma, dbeta, workspace, workspace_bytes, stream,
                                   &add);
}

int fewbit_hipx_add_rms_norm_forward(int dtype, const void *x, const void *residual, size_t rows, size_t width, const void *gamma, double eps, int bits,
                                     uint64_t seed, const uint64_t *seed_device, uint32_t threshold, void *y, void *h_out, float *rstd, uint8_t *state,
                                     size_t state_bytes, float *xhat_out, void *stream) {
    const ForwardFusion add{residual, h_out, threshold, 0.0f};
    return forward_call<kUncentred>("add_rms_norm_forward", dtype, x, rows, width, gamma, nullptr, eps, bits, seed, seed_device, y, rstd, state, state_bytes, xhat_out,
                                    stream, &add);
}

int fewbit_hipx_add_rms_norm_backward(int dtype, const void *gy, const void *gh, const uint8_t *state, const float *rstd, const void *gamma, size_t rows, size_t width,
                                      int bits, uint64_t seed, const uint64_t *seed_device, uint32_t threshold, void *dres, void *dbranch, float *dgamma,
                                      void *workspace, size_t workspace_bytes, void *stream) {
    const BackwardFusion add{gh, dbranch, sketch::key_of(seed), reinterpret_cast<const Key *>(seed_device), threshold, 0.0f};
    return backward_call<kUncentred>("add_rms_norm_backward", dtype, gy, state, rstd, gamma, rows, width, bits, dres, dgamma, nullptr, workspace, workspace_bytes,
                                     stream, &add);
}

}  // extern "C"
#endif  // FEWBIT_NORM_TU == 0
