// fewbit_mxrows.h -- what the norms that keep their normalized rows as OCP-MX cells share (fewbit_mxnorm.hip: the RMS norm; fewbit_mxlnorm.hip: the
// layer norm): the geometry of a workgroup that owns whole row blocks, the fixed-order lane sums, the load role (eight consecutive columns of one
// row) and the rounding role of mx::pack_kernel on one LDS tile, the cells between the buffer and LDS, what their entry points refuse alike, and
// the mask and the sum of the pairs that take residual + dropout(x) in front of the norm.
// Every device function here is inlined into its kernel; the text is the one fewbit_mxnorm.hip had, moved as it was.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

#include "fewbit_hipx.h"
#include "fewbit_mxdef.h"

#pragma clang fp contract(off)

namespace fewbit_hip {
namespace quant {
namespace mxrows {

constexpr int kRows = mx::kCellRows, kOctets = mx::kOctets, kTileCols = 64;                   // the tile of mx::pack_kernel
constexpr int kGroupThreads = 256, kGroups = 4, kThreads = kGroups * kGroupThreads, kWaves = kThreads / 64;
constexpr size_t kMaxWidth = 8192;
constexpr size_t kMaxGridForward = size_t{1} << 16, kMaxGridBackward = 512;
constexpr int kMirrorSixteen = 0x140;       // row_mirror

inline bool known_shape(size_t rows, size_t width) { return rows >= 1 && width >= 1 && width <= kMaxWidth && rows <= kMaxCount / width; }
inline size_t backward_grid(size_t rows) { const size_t blocks = mx::blocks_of(rows); return blocks < kMaxGridBackward ? blocks : kMaxGridBackward; }

__device__ __forceinline__ float sqrt_rn(float v) { return __fsqrt_rn(v); }
template <int CTRL> __device__ __forceinline__ float sum_step(float v) {
    return add_rn(v, __builtin_bit_cast(float, lane_move<CTRL>(__builtin_bit_cast(int, v))));
}
__device__ __forceinline__ float lane_value(float v, int lane) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane)); }
// the sum of v over the eight lanes of a row of a tile (lane ^ 1, lane ^ 2, the other quad), the same bits in each of them
__device__ __forceinline__ float eight_sum(float v) {
    v = sum_step<kSwapPairs>(v);
    v = sum_step<kSwapHalves>(v);
    return sum_step<kMirrorEight>(v);
}
// the sum of v over a wave, the order of norm::row_sum<64>
__device__ __forceinline__ float wave_sum(float v) {
    v = sum_step<kMirrorSixteen>(eight_sum(v));
    return add_rn(add_rn(lane_value(v, 0), lane_value(v, 16)), add_rn(lane_value(v, 32), lane_value(v, 48)));
}

// ---- the load role: eight consecutive columns of one row (the text of mxglu::load_piece / store_piece) -------------------------------------------
template <int DT>
__device__ __forceinline__ void load_piece(const typename Elem<DT>::type *src, size_t ld, bool vec, size_t r, size_t col, size_t rows, size_t width,
                                           typename Elem<DT>::type (&raw)[kBlock]) {
    using T = typename Elem<DT>::type;
    if (vec && r < rows && col + kBlock <= width) {
        load8<DT>(src + r * ld + col, raw);
    } else {
#pragma unroll
        for (int k = 0; k < kBlock; ++k) raw[k] = r < rows && col + k < width ? src[r * ld + col + k] : T{0};
    }
}
template <int DT>
__device__ __forceinline__ void store_piece(typename Elem<DT>::type *dst, size_t ld, bool vec, size_t r, size_t col, size_t rows, size_t width,
                                            const typename Elem<DT>::type (&raw)[kBlock]) {
    if (r >= rows) return;
    if (vec && col + kBlock <= width) {
        store8<DT>(dst + r * ld + col, raw);
    } else {
#pragma unroll
        for (int k = 0; k < kBlock; ++k)
            if (col + k < width) dst[r * ld + col + k] = raw[k];
    }
}

// ---- the sum of a seed in front of a norm, h = residual + dropout(x), in the load role (the fused pairs of both units) -------------------------------
// the 16 mask bits of the eight elements of the piece (r, col .. col + 7), flat block (r width + col) / 8 where width % 8 == 0; threshold 0 keeps
// everything and draws nothing (the text of norm::mask_words)
__device__ __forceinline__ void piece_mask(size_t r, size_t col, size_t width, Key key, uint32_t threshold, uint32_t (&w)[4]) {
    w[0] = w[1] = w[2] = w[3] = ~0u;
    if (threshold != 0) block_words<kMaskDomain>((static_cast<uint64_t>(r) * width + col) / kBlock, key, w);
}
// h = keep ? narrow(widen(x) scale + widen(res)) : res, and dbranch = keep ? narrow(widen(dres) scale) : +0 -- `one<DT, true>` and `one<DT, false>`
// of fewbit_dropout.hip as fewbit_norm.hip writes them on widen / narrow: the product and the sum are fp32 values of their own (an fp16 operand's
// conversion, the arithmetic and the rounding must not meet in one v_fma_mix*, which is one step off at the ties)
template <int DT> __device__ __forceinline__ typename Elem<DT>::type dropped_sum(typename Elem<DT>::type x, typename Elem<DT>::type res, bool keep, float scale) {
    float v = mul_rn(float_of_bits(widen<DT>(x)), scale);
    if constexpr (DT == FEWBIT_F16) asm("" : "+v"(v));
    v = add_rn(v, float_of_bits(widen<DT>(res)));
    return keep ? narrow<DT>(v) : res;
}
template <int DT> __device__ __forceinline__ typename Elem<DT>::type dropped_gradient(typename Elem<DT>::type dres, bool keep, float scale) {
    const float v = mul_rn(float_of_bits(widen<DT>(dres)), scale);
    return keep ? narrow<DT>(v) : typename Elem<DT>::type{0};
}
// the eight h of the piece (r, col .. col + 7) as rounded to the dtype: two loads and one draw (outside the matrix: +0).  Args: a unit's AddForwardArgs
template <int DT, class Args>
__device__ __forceinline__ void sum_piece(const Args &a, Key mask_key, size_t r, size_t col, typename Elem<DT>::type (&h)[kBlock]) {
    using T = typename Elem<DT>::type;
    T rx[kBlock], rr[kBlock];
    load_piece<DT>(static_cast<const T *>(a.x), a.ld_x, a.vec_x, r, col, a.rows, a.width, rx);
    load_piece<DT>(static_cast<const T *>(a.residual), a.ld_res, a.vec_res, r, col, a.rows, a.width, rr);
    uint32_t w[4];
    piece_mask(r, col, a.width, mask_key, a.threshold, w);
#pragma unroll
    for (int k = 0; k < kBlock; ++k) h[k] = dropped_sum<DT>(rx[k], rr[k], mask_bits(w, k) >= a.threshold, a.scale);
}
// a + b as torch adds two tensors of the dtype: both widened, the fp32 sum rounded once
template <int DT> __device__ __forceinline__ typename Elem<DT>::type added(typename Elem<DT>::type a, typename Elem<DT>::type b) {
    return narrow<DT>(add_rn(float_of_bits(widen<DT>(a)), float_of_bits(widen<DT>(b))));
}

// ---- the rounding role of mx::pack_kernel on one LDS tile of fp32 bits, in its two halves: the caller's barrier lies between them ---------------
__device__ __forceinline__ void column_amax(const uint32_t (&tile)[kRows][kTileCols], int c, int o, uint32_t (&v)[kBlock], uint32_t (&amax_s)[kOctets][kTileCols]) {
    uint32_t amax = 0;
#pragma unroll
    for (int k = 0; k < kBlock; ++k) {
        v[k] = tile[kBlock * o + k][c];
        const uint32_t m = v[k] & 0x7fffffffu;
        amax = m > amax ? m : amax;
    }
    amax_s[o][c] = amax;
}
// -> the octet's codes in the LDS image of the tile's cells, the scale byte of column `col` of block b into `out` (the buffer)
template <int FMT>
__device__ __forceinline__ void column_codes(const uint32_t (&v)[kBlock], const uint32_t (&amax_s)[kOctets][kTileCols], int c, int o, size_t b, size_t col, size_t width,
                                             Key key, uint64_t *image, uint8_t *out) {
    uint32_t amax = 0;
#pragma unroll
    for (int k = 0; k < kOctets; ++k) amax = amax_s[k][c] > amax ? amax_s[k][c] : amax;
    const bool bad = amax >= 0x7f800000u;
    const int e = bad ? 128 : mx::scale_of_amax<FMT>(amax);
    uint32_t w[4];
    mx::octet_words(b, col, width, o, mx::kKeptDomain, key, w);
    const uint64_t word = mx::octet_codes<FMT>(v, e, bad, w);
    if constexpr (FMT == 4) reinterpret_cast<uint32_t *>(image)[kOctets * c + o] = static_cast<uint32_t>(word);
    else {
        uint16_t *at = reinterpret_cast<uint16_t *>(image) + 12 * c + 3 * o;
        at[0] = static_cast<uint16_t>(word), at[1] = static_cast<uint16_t>(word >> 16), at[2] = static_cast<uint16_t>(word >> 32);
    }
    if (o == 0 && col < width) out[b * width + col] = static_cast<uint8_t>(e + 127);
}
// the tile's cells, `cols` of them, between the buffer and LDS: 8-byte pieces, consecutive lanes consecutive pieces (u: the lane of the group)
template <int FMT> __device__ __forceinline__ void store_cells(const uint64_t *image, uint8_t *codes, size_t b, size_t j0, size_t width, size_t cols, int u) {
    if (8 * static_cast<size_t>(u) < cols * mx::cell_bytes(FMT)) reinterpret_cast<uint64_t *>(codes + (b * width + j0) * mx::cell_bytes(FMT))[u] = image[u];
}
template <int FMT> __device__ __forceinline__ void load_cells(uint64_t *image, const uint8_t *codes, size_t b, size_t j0, size_t width, size_t cols, int u) {
    if (8 * static_cast<size_t>(u) < cols * mx::cell_bytes(FMT)) image[u] = reinterpret_cast<const uint64_t *>(codes + (b * width + j0) * mx::cell_bytes(FMT))[u];
}
// element `row` of the cell of tile column `c` in an LDS image, as mx::unpack_kernel reads it
template <int FMT> __device__ __forceinline__ uint32_t code_at(const uint64_t *image, int c, int row) {
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(image);
    const size_t bit = mx::cell_bytes(FMT) * 8 * c + FMT * row;
    uint32_t two = bytes[bit / 8];
    if (bit % 8 + FMT > 8) two |= static_cast<uint32_t>(bytes[bit / 8 + 1]) << 8;                  // (fp6 only, and never for a cell's last code)
    return (two >> (bit % 8)) & ((1u << FMT) - 1u);
}

// dst[c] = the workgroups' sums of column c.  A workgroup of 16 waves takes 64 columns: wave w adds the rows [w per, (w + 1) per) of `partials` (row p
// at partials + p * stride) in ascending order, per = ceil(parts / 16), and the waves' results are added in ascending order -- the rows in ascending
// order, associated by sixteenths, so that 16 loads of a column are in flight and not one.  (the body of the column-sum launches of both norms)
__device__ __forceinline__ void add_partials(const float *__restrict__ partials, size_t parts, size_t stride, size_t width, size_t chunk, float *__restrict__ dst,
                                             float (&waves)[kWaves][kTileCols]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t c = chunk * kTileCols + lane;
    const size_t per = (parts + kWaves - 1) / kWaves, from = wave * per, to = from + per < parts ? from + per : parts;
    float sum = 0.0f;
    if (c < width && from < parts) {
        sum = partials[from * stride + c];
#pragma unroll 8
        for (size_t p = from + 1; p < to; ++p) sum = add_rn(sum, partials[p * stride + c]);
    }
    waves[wave][lane] = sum;
    __syncthreads();
    if (wave == 0 && c < width) {
        float total = waves[0][lane];
        for (size_t w = 1; w < static_cast<size_t>(kWaves) && w * per < parts; ++w) total = add_rn(total, waves[w][lane]);
        dst[c] = total;
    }
}

// what the entry points refuse alike, in the order of mxglu::check_call
inline int check_call(const char *name, int dtype, int format, const void *seed_device, size_t rows, size_t width) {
    if (const int rc = check_dtype(name, dtype)) return rc;
    if (format != 4 && format != 6) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: format = %d is not 4 (fp4) or 6 (fp6)", name, format);
    if (const int rc = check_seed_word(name, seed_device)) return rc;
    if (rows == 0) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: rows = 0", name);
    if (width == 0 || width > kMaxWidth) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: width = %zu is not in 1 .. %zu", name, width, kMaxWidth);
    if (rows > kMaxCount / width) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: rows * width = %zu * %zu is beyond 2^36", name, rows, width);
    return FEWBIT_OK;
}
inline int check_aligned16(const char *name, const char *what, const void *p) {
    return !misaligned(p, 16) ? FEWBIT_OK : fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: %s must be 16-byte aligned", name, what);
}
// what the fused pairs refuse on top: a threshold beyond 65536, and a mask where a lane's piece is no mask block
inline int check_mask(const char *name, uint32_t threshold, size_t width) {
    if (threshold > kOne) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: threshold = %u is beyond 65536", name, threshold);
    if (threshold != 0 && width % kBlock != 0)
        return fail(FEWBIT_ERR_UNSUPPORTED, "%s: a mask (threshold = %u) needs a width that is a multiple of 8, not %zu", name, threshold, width);
    return FEWBIT_OK;
}
// whether two rows x width matrices of `item`-byte elements (either may be absent) share a byte.  Exact where the row strides agree (column
// blocks of one buffer do not meet); with different strides every meeting of the two spans counts.
inline bool matrices_meet(const void *p, size_t ld_p, const void *q, size_t ld_q, size_t rows, size_t width, size_t item) {
    if (p == nullptr || q == nullptr) return false;
    uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    if (a > b) std::swap(a, b), std::swap(ld_p, ld_q);
    if (a + ((rows - 1) * ld_p + width) * item <= b) return false;
    if (ld_p != ld_q) return true;
    const size_t pitch = ld_p * item, row = width * item, off = (b - a) % pitch;
    return off < row || off + row > pitch;
}
// whether 16-byte pieces serve a tensor (an absent one: they would)
inline bool wide(const void *p, size_t ld, int dtype) { return !misaligned(p, 16) && ld * size_of(dtype) % 16 == 0; }

template <class F> void pick_kernel(int dtype, int format, F &&f) {
    pick_dtype(dtype, [&](auto dt) { pick<4, 6>(format, [&](auto fmt) { f(dt, fmt); }); });
}

}  // namespace mxrows
}  // namespace quant
}  // namespace fewbit_hip
