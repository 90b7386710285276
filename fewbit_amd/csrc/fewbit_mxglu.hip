// fewbit_mxglu.hip -- the product of a gated MLP, y = act(gate) * up, that keeps BOTH inputs as OCP-MX cells down their columns, and its backward, which
// writes the two gradients a second time as fp8 cells and the rebuilt product as cells only, on gfx950; part of the companion library
// libfewbit_hipx.so (include/fewbit_hipx.h, "The gate and the up as row blocks"):
//
//     mx_glu_forward    gate, up (rows x width, own row strides) -> y (the bytes of fewbit_hipx_glu_forward) and a state of two mx_pack buffers  ONE launch
//     mx_glu_backward   gy and that state -> d_gate, d_up in `dtype`, and three mx_pack buffers: d_gate and d_up as fp8 'grad' cells, y^ = act(g^) * u^
//                       as fp4 / fp6 'kept' cells -- the operands of three mx_wgrad calls; y^ itself is never written                          ONE launch
//
// Every buffer is bit for bit what mx_pack writes from the tensor in `dtype` with that buffer's seed: the format is fewbit_mxdef.h's (scale_of_amax,
// octet_words, octet_codes, decode, used as they are), the arithmetic of the product is fewbit_gluact.h's (the text of fewbit_glu.hip).  What is new
// here is the walk: both kernels take the tile of mx::pack_kernel, so that the transpose through LDS that a stand-alone pack of d_gate, d_up and y^
// would each pay in a launch of its own is paid once, on values that are still in the workgroup.
//   workgroup  256 lanes take a tile of 32 rows (ONE row block b) x 64 columns; the grid walks the tiles.
//   load role  lane t: row t / 8, columns 8 (t % 8) .. + 7 of the tile, one 16-byte piece per tensor (two at fp32) where its pointer and stride allow
//              and the piece is inside the matrix, element accesses otherwise -- the same values either way.  Rows and columns outside count as +0.
//              forward: y from gate and up, both raw values -> two LDS tiles.
//              backward: the tile's two cell images and scale bytes come into LDS by 8-byte pieces first; the lane decodes its eight g^ and u^ as
//              mx::unpack_kernel does, loads gy, forms d_gate, d_up and y^, rounds each ONCE to `dtype`, stores the two gradients and puts the three
//              ROUNDED values into three LDS tiles.
//   round role lane t: column t % 64, row octet t / 64 (wave-uniform), the role of mx::pack_kernel on each LDS tile: eight values down the column, the
//              four octets' amax meet through LDS, one Philox call per tensor with that tensor's key, eight codes -> the LDS image of the cells.
//   store      a tile's cells are contiguous in each buffer: 8-byte pieces, consecutive lanes consecutive pieces; the scale bytes from the first wave.
//   barriers   forward 3 a tile, backward 5; the last one of a round also keeps the next round's writes behind this round's reads.
//   poison     a state cell with scale byte 0xFF of EITHER input makes d_gate, d_up and y^ NaN on its 32 rows of that column; the cells written from
//              them are poisoned by the ordinary rule of the pack.  No atomics, no workspace: the same arguments give the same bytes.
// Roofline class: memory (forward reads 2 and writes 1 element plus 2 cells, backward reads 1 element plus 2 cells and writes 2 elements plus 3 cells).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fewbit_hipx.h"
// (fewbit_mxdef.h in front of fewbit_device.h: the definition names kBlock, and fewbit_device.h declares another one in fewbit_hip)
#include "fewbit_mxdef.h"
#include "fewbit_device.h"
#include "fewbit_gluact.h"

#pragma clang fp contract(off)

namespace fewbit_hip {
namespace quant {
namespace mxglu {

using glu::act_of;
using glu::slope_of;

constexpr int kRows = mx::kCellRows, kOctets = mx::kOctets, kTileCols = 64, kThreads = 256;    // the tile of mx::pack_kernel
constexpr size_t kMaxTiles = size_t{1} << 20;             // workgroups; beyond that a workgroup walks on by the grid's width

// one buffer's place in a state: the second starts at the first's size filled up to a multiple of 16, so that either is an aligned mx_pack buffer
inline size_t half_of(size_t rows, size_t width, int format) { return (mx::bytes_of(rows, width, format) + 15) / 16 * 16; }

struct ForwardArgs {
    const void *gate, *up;
    size_t ld_gate, ld_up, rows, width;
    Key key_gate, key_up;
    const Key *device;                      // nullptr, or the two keys in device memory
    void *y;
    size_t ld_y;
    uint8_t *state;
    size_t half, across, count;
    bool vec_gate, vec_up, vec_y;
};
struct BackwardArgs {
    const void *gy;
    size_t ld_gy;
    const uint8_t *state;
    size_t half, rows, width;
    Key key_dgate, key_dup, key_product;
    const Key *device;                      // nullptr, or the three keys in device memory
    void *d_gate, *d_up;                    // either may be absent, and so may each of the three cell buffers: what is absent is not written
    size_t ld_dgate, ld_dup;
    uint8_t *d_gate_cells, *d_up_cells, *product_cells;
    size_t across, count;
    bool vec_gy, vec_dgate, vec_dup;
};

// ---- the load role: eight consecutive columns of one row ----------------------------------------------------------------------------------------------
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

// ---- the rounding role of mx::pack_kernel on one LDS tile, in its two halves: the caller's barrier lies between them ---------------------------------
template <int DT>
__device__ __forceinline__ void column_amax(const typename Elem<DT>::type (&tile)[kRows][kTileCols], int c, int o, uint32_t (&v)[kBlock],
                                            uint32_t (&amax_s)[kOctets][kTileCols]) {
    uint32_t amax = 0;
#pragma unroll
    for (int k = 0; k < kBlock; ++k) {
        v[k] = widen<DT>(tile[kBlock * o + k][c]);
        const uint32_t m = v[k] & 0x7fffffffu;
        amax = m > amax ? m : amax;
    }
    amax_s[o][c] = amax;
}
// -> the octet's codes in the LDS image of the tile's cells, the scale byte of column `col` of block b into `out` (the buffer)
template <int FMT>
__device__ __forceinline__ void column_codes(const uint32_t (&v)[kBlock], const uint32_t (&amax_s)[kOctets][kTileCols], int c, int o, size_t b, size_t col, size_t width,
                                             uint32_t domain, Key key, uint64_t *image, uint8_t *out) {
    uint32_t amax = 0;
#pragma unroll
    for (int k = 0; k < kOctets; ++k) amax = amax_s[k][c] > amax ? amax_s[k][c] : amax;
    const bool bad = amax >= 0x7f800000u;
    const int e = bad ? 128 : mx::scale_of_amax<FMT>(amax);
    uint32_t w[4];
    mx::octet_words(b, col, width, o, domain, key, w);
    const uint64_t word = mx::octet_codes<FMT>(v, e, bad, w);
    if constexpr (FMT == 4) reinterpret_cast<uint32_t *>(image)[kOctets * c + o] = static_cast<uint32_t>(word);
    else if constexpr (FMT == 8) image[kOctets * c + o] = word;
    else {
        uint16_t *at = reinterpret_cast<uint16_t *>(image) + 12 * c + 3 * o;
        at[0] = static_cast<uint16_t>(word), at[1] = static_cast<uint16_t>(word >> 16), at[2] = static_cast<uint16_t>(word >> 32);
    }
    if (o == 0 && col < width) out[b * width + col] = static_cast<uint8_t>(e + 127);
}
// the tile's cells, `cols` of them, between the buffer and LDS: 8-byte pieces, consecutive lanes consecutive pieces
template <int FMT> __device__ __forceinline__ void store_cells(const uint64_t *image, uint8_t *codes, size_t b, size_t j0, size_t width, size_t cols, int t) {
    if (8 * static_cast<size_t>(t) < cols * mx::cell_bytes(FMT)) reinterpret_cast<uint64_t *>(codes + (b * width + j0) * mx::cell_bytes(FMT))[t] = image[t];
}
template <int FMT> __device__ __forceinline__ void load_cells(uint64_t *image, const uint8_t *codes, size_t b, size_t j0, size_t width, size_t cols, int t) {
    if (8 * static_cast<size_t>(t) < cols * mx::cell_bytes(FMT)) image[t] = reinterpret_cast<const uint64_t *>(codes + (b * width + j0) * mx::cell_bytes(FMT))[t];
}
// element `row` of the cell of tile column `c` in an LDS image, as mx::unpack_kernel reads it
template <int FMT> __device__ __forceinline__ uint32_t code_at(const uint64_t *image, int c, int row) {
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(image);
    const size_t bit = mx::cell_bytes(FMT) * 8 * c + FMT * row;
    uint32_t two = bytes[bit / 8];
    if (bit % 8 + FMT > 8) two |= static_cast<uint32_t>(bytes[bit / 8 + 1]) << 8;                  // (fp6 only, and never for a cell's last code)
    return (two >> (bit % 8)) & ((1u << FMT) - 1u);
}

template <int DT, int ACT, int FMT>
__global__ __launch_bounds__(kThreads) void forward_kernel(ForwardArgs a) {
    using T = typename Elem<DT>::type;
    constexpr bool kFast = DT != FEWBIT_F32;
    constexpr size_t kCell = mx::cell_bytes(FMT);
    __shared__ T tile[2][kRows][kTileCols];                // 0: gate, 1: up
    __shared__ uint32_t amax_s[2][kOctets][kTileCols];
    __shared__ uint64_t image[2][kTileCols * kCell / 8];
    const T *gate = static_cast<const T *>(a.gate), *up = static_cast<const T *>(a.up);
    T *y = static_cast<T *>(a.y);
    Key key_gate = a.key_gate, key_up = a.key_up;
    if (a.device != nullptr) key_gate = a.device[0], key_up = a.device[1];
    const size_t rows = a.rows, width = a.width;
    uint8_t *second = a.state + a.half;
    uint8_t *codes_gate = a.state + mx::codes_offset(rows, width), *codes_up = second + mx::codes_offset(rows, width);
    const int t = threadIdx.x;
    const int lrow = t >> 3, lcol = 8 * (t & 7);          // the load role
    const int c = t & (kTileCols - 1), o = t >> 6;        // the rounding role: column c, row octet o
    for (size_t tl = blockIdx.x; tl < a.count; tl += gridDim.x) {
        const size_t b = tl / a.across, j0 = (tl % a.across) * kTileCols;
        const size_t r = kRows * b + lrow, col = j0 + lcol;
        T rg[kBlock], ru[kBlock], ry[kBlock];
        load_piece<DT>(gate, a.ld_gate, a.vec_gate, r, col, rows, width, rg);
        load_piece<DT>(up, a.ld_up, a.vec_up, r, col, rows, width, ru);
#pragma unroll
        for (int k = 0; k < kBlock; ++k) {
            // (the expression of glu_forward_kernel: act in fp32, one product, rounded once)
            ry[k] = narrow<DT>(mul_rn(act_of<ACT, kFast>(float_of_bits(widen<DT>(rg[k]))), float_of_bits(widen<DT>(ru[k]))));
            tile[0][lrow][lcol + k] = rg[k];
            tile[1][lrow][lcol + k] = ru[k];
        }
        store_piece<DT>(y, a.ld_y, a.vec_y, r, col, rows, width, ry);
        __syncthreads();
        uint32_t vg[kBlock], vu[kBlock];
        column_amax<DT>(tile[0], c, o, vg, amax_s[0]);
        column_amax<DT>(tile[1], c, o, vu, amax_s[1]);
        __syncthreads();
        column_codes<FMT>(vg, amax_s[0], c, o, b, j0 + c, width, mx::kKeptDomain, key_gate, image[0], a.state);
        column_codes<FMT>(vu, amax_s[1], c, o, b, j0 + c, width, mx::kKeptDomain, key_up, image[1], second);
        __syncthreads();
        const size_t cols = width - j0 < static_cast<size_t>(kTileCols) ? width - j0 : kTileCols;
        store_cells<FMT>(image[0], codes_gate, b, j0, width, cols, t);
        store_cells<FMT>(image[1], codes_up, b, j0, width, cols, t);
        // (the next round writes `tile` behind this round's second barrier's reads, `amax_s` and `image` behind its third: no barrier here)
    }
}

template <int DT, int ACT, int FMT>
__global__ __launch_bounds__(kThreads) void backward_kernel(BackwardArgs a) {
    using T = typename Elem<DT>::type;
    constexpr bool kFast = DT != FEWBIT_F32;
    constexpr size_t kCell = mx::cell_bytes(FMT);
    __shared__ uint64_t kept_image[2][kTileCols * kCell / 8];                  // 0: gate, 1: up
    __shared__ uint8_t scale_s[2][kTileCols];
    __shared__ T tile[3][kRows][kTileCols];                                     // 0: d_gate, 1: d_up, 2: y^, each rounded to T
    __shared__ uint32_t amax_s[3][kOctets][kTileCols];
    __shared__ uint64_t grad_image[2][kTileCols * mx::cell_bytes(8) / 8];
    __shared__ uint64_t product_image[kTileCols * kCell / 8];
    const T *gy = static_cast<const T *>(a.gy);
    T *d_gate = static_cast<T *>(a.d_gate), *d_up = static_cast<T *>(a.d_up);
    Key key_dgate = a.key_dgate, key_dup = a.key_dup, key_product = a.key_product;
    if (a.device != nullptr) key_dgate = a.device[0], key_dup = a.device[1], key_product = a.device[2];
    const size_t rows = a.rows, width = a.width;
    const uint8_t *second = a.state + a.half;
    const uint8_t *codes_gate = a.state + mx::codes_offset(rows, width), *codes_up = second + mx::codes_offset(rows, width);
    const size_t grad_codes = mx::codes_offset(rows, width);                     // (the offset of the codes is the same at every format)
    const bool cells_dgate = a.d_gate_cells != nullptr, cells_dup = a.d_up_cells != nullptr, cells_product = a.product_cells != nullptr;
    const int t = threadIdx.x;
    const int lrow = t >> 3, lcol = 8 * (t & 7);          // the load role
    const int c = t & (kTileCols - 1), o = t >> 6;        // the rounding role: column c, row octet o
    for (size_t tl = blockIdx.x; tl < a.count; tl += gridDim.x) {
        const size_t b = tl / a.across, j0 = (tl % a.across) * kTileCols;
        const size_t cols = width - j0 < static_cast<size_t>(kTileCols) ? width - j0 : kTileCols;
        load_cells<FMT>(kept_image[0], codes_gate, b, j0, width, cols, t);
        load_cells<FMT>(kept_image[1], codes_up, b, j0, width, cols, t);
        if (static_cast<size_t>(t) < cols) scale_s[0][t] = a.state[b * width + j0 + t], scale_s[1][t] = second[b * width + j0 + t];
        __syncthreads();
        const size_t r = kRows * b + lrow, col = j0 + lcol;
        T rgy[kBlock], rdg[kBlock], rdu[kBlock], rpr[kBlock];
        load_piece<DT>(gy, a.ld_gy, a.vec_gy, r, col, rows, width, rgy);
#pragma unroll
        for (int k = 0; k < kBlock; ++k) {
            const bool inside = r < rows && lcol + k < static_cast<int>(cols);
            const uint32_t scale_g = inside ? scale_s[0][lcol + k] : 127u, scale_u = inside ? scale_s[1][lcol + k] : 127u;
            const float g = inside ? mx::decode<FMT>(code_at<FMT>(kept_image[0], lcol + k, lrow), scale_g) : 0.0f;
            const float u = inside ? mx::decode<FMT>(code_at<FMT>(kept_image[1], lcol + k, lrow), scale_u) : 0.0f;
            // a poisoned cell of EITHER input: every output is NaN on its rows of the column (said here: the clamps of the activations swallow a NaN)
            const bool poisoned = scale_g == mx::kPoisonScale || scale_u == mx::kPoisonScale;
            const float upstream = float_of_bits(widen<DT>(rgy[k]));
            // (the expressions of glu_backward_kernel<PRODUCT>)
            const float value = act_of<ACT, kFast>(g);
            const float du = mul_rn(upstream, value);
            const float dg = mul_rn(mul_rn(upstream, u), slope_of<ACT, kFast>(g));
            const float pr = mul_rn(value, u);
            rdg[k] = inside ? narrow<DT>(poisoned ? float_of_bits(kNaN) : dg) : T{0};
            rdu[k] = inside ? narrow<DT>(poisoned ? float_of_bits(kNaN) : du) : T{0};
            rpr[k] = inside ? narrow<DT>(poisoned ? float_of_bits(kNaN) : pr) : T{0};
            tile[0][lrow][lcol + k] = rdg[k];
            tile[1][lrow][lcol + k] = rdu[k];
            tile[2][lrow][lcol + k] = rpr[k];
        }
        if (d_gate != nullptr) store_piece<DT>(d_gate, a.ld_dgate, a.vec_dgate, r, col, rows, width, rdg);
        if (d_up != nullptr) store_piece<DT>(d_up, a.ld_dup, a.vec_dup, r, col, rows, width, rdu);
        __syncthreads();
        uint32_t vdg[kBlock], vdu[kBlock], vpr[kBlock];
        column_amax<DT>(tile[0], c, o, vdg, amax_s[0]);
        column_amax<DT>(tile[1], c, o, vdu, amax_s[1]);
        column_amax<DT>(tile[2], c, o, vpr, amax_s[2]);
        __syncthreads();
        if (cells_dgate) column_codes<8>(vdg, amax_s[0], c, o, b, j0 + c, width, mx::kGradDomain, key_dgate, grad_image[0], a.d_gate_cells);
        if (cells_dup) column_codes<8>(vdu, amax_s[1], c, o, b, j0 + c, width, mx::kGradDomain, key_dup, grad_image[1], a.d_up_cells);
        if (cells_product) column_codes<FMT>(vpr, amax_s[2], c, o, b, j0 + c, width, mx::kKeptDomain, key_product, product_image, a.product_cells);
        __syncthreads();
        if (cells_dgate) store_cells<8>(grad_image[0], a.d_gate_cells + grad_codes, b, j0, width, cols, t);
        if (cells_dup) store_cells<8>(grad_image[1], a.d_up_cells + grad_codes, b, j0, width, cols, t);
        if (cells_product) store_cells<FMT>(product_image, a.product_cells + grad_codes, b, j0, width, cols, t);
        __syncthreads();                                   // (the next round's cell images and tiles behind this round's reads)
    }
}

inline unsigned grid_of(size_t count) { return static_cast<unsigned>(count < kMaxTiles ? count : kMaxTiles); }

// what both entry points refuse alike, in the order of fewbit_hipx_mx_pack, the pointers and the buffers apart; 1: no elements, nothing to do
inline int check_call(const char *name, int dtype, int act, int format, const void *seed_device, size_t rows, size_t width) {
    if (const int rc = check_dtype(name, dtype)) return rc;
    if (act != FEWBIT_SILU && act != FEWBIT_GELU) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: activation %d is neither FEWBIT_SILU nor FEWBIT_GELU", name, act);
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
// whether 16-byte pieces serve a tensor (an absent one: they would)
inline bool wide(const void *p, size_t ld, int dtype) { return !misaligned(p, 16) && ld * size_of(dtype) % 16 == 0; }

template <class F> void pick_kernel(int dtype, int act, int format, F &&f) {
    pick_dtype(dtype, [&](auto dt) { pick<FEWBIT_SILU, FEWBIT_GELU>(act, [&](auto ac) { pick<4, 6>(format, [&](auto fmt) { f(dt, ac, fmt); }); }); });
}

}  // namespace mxglu
}  // namespace quant
}  // namespace fewbit_hip

using namespace fewbit_hip::quant;
using fewbit_hip::sketch::key_of;

extern "C" {

size_t fewbit_hipx_mx_glu_state_bytes(size_t rows, size_t width, int format) {
    return (format == 4 || format == 6) && fewbit_hip::mx::bytes_of(rows, width, format) != 0 ? 2 * mxglu::half_of(rows, width, format) : 0;
}

int fewbit_hipx_mx_glu_forward(int dtype, int act, const void *gate, size_t ld_gate, const void *up, size_t ld_up, size_t rows, size_t width, int format,
                               uint64_t seed_gate, uint64_t seed_up, const uint64_t *seed_device, void *y, size_t ld_y, uint8_t *state, size_t state_bytes,
                               void *stream) {
    using namespace mxglu;
    const char *name = "mx_glu_forward";
    if (const int rc = check_call(name, dtype, act, format, seed_device, rows, width)) return rc < 0 ? rc : FEWBIT_OK;
    if (gate == nullptr || up == nullptr || y == nullptr || state == nullptr) return refuse_null(name);
    if (ld_gate < width || ld_up < width || ld_y < width)
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: a row stride ld (%zu, %zu, %zu) must be at least width = %zu", name, ld_gate, ld_up, ld_y, width);
    const size_t item = size_of(dtype);
    if (misaligned(gate, item) || misaligned(up, item) || misaligned(y, item))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: gate, up and y must be aligned to their element size", name);
    if (const int rc = check_aligned16(name, "state", state)) return rc;
    const size_t half = half_of(rows, width, format);
    if (const int rc = check_bytes(name, "state", state_bytes, 2 * half)) return rc;
    const size_t across = (width + kTileCols - 1) / kTileCols, count = across * fewbit_hip::mx::blocks_of(rows);
    const ForwardArgs a{gate, up, ld_gate, ld_up, rows, width, key_of(seed_gate), key_of(seed_up), reinterpret_cast<const Key *>(seed_device), y, ld_y, state, half,
                        across, count, wide(gate, ld_gate, dtype), wide(up, ld_up, dtype), wide(y, ld_y, dtype)};
    pick_kernel(dtype, act, format, [&](auto dt, auto ac, auto fmt) {
        hipLaunchKernelGGL((forward_kernel<dt(), ac(), fmt()>), dim3(grid_of(count)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

int fewbit_hipx_mx_glu_backward(int dtype, int act, const void *gy, size_t ld_gy, const uint8_t *state, size_t state_bytes, size_t rows, size_t width, int format,
                                uint64_t seed_dgate, uint64_t seed_dup, uint64_t seed_product, const uint64_t *seed_device, void *d_gate, size_t ld_dgate,
                                void *d_up, size_t ld_dup, uint8_t *d_gate_cells, uint8_t *d_up_cells, uint8_t *product_cells, void *stream) {
    using namespace mxglu;
    const char *name = "mx_glu_backward";
    if (const int rc = check_call(name, dtype, act, format, seed_device, rows, width)) return rc < 0 ? rc : FEWBIT_OK;
    if (gy == nullptr || state == nullptr) return refuse_null(name);
    if (ld_gy < width || (d_gate != nullptr && ld_dgate < width) || (d_up != nullptr && ld_dup < width))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: a row stride ld (%zu, %zu, %zu) must be at least width = %zu", name, ld_gy, ld_dgate, ld_dup, width);
    const size_t item = size_of(dtype);
    if (misaligned(gy, item) || misaligned(d_gate, item) || misaligned(d_up, item))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: gy, d_gate and d_up must be aligned to their element size", name);
    if (const int rc = check_aligned16(name, "state", state)) return rc;
    if (const int rc = check_aligned16(name, "d_gate_cells", d_gate_cells)) return rc;
    if (const int rc = check_aligned16(name, "d_up_cells", d_up_cells)) return rc;
    if (const int rc = check_aligned16(name, "product_cells", product_cells)) return rc;
    const size_t half = half_of(rows, width, format);
    if (const int rc = check_bytes(name, "state", state_bytes, 2 * half)) return rc;
    if (d_gate == nullptr && d_up == nullptr && d_gate_cells == nullptr && d_up_cells == nullptr && product_cells == nullptr) return FEWBIT_OK;
    const size_t across = (width + kTileCols - 1) / kTileCols, count = across * fewbit_hip::mx::blocks_of(rows);
    const BackwardArgs a{gy, ld_gy, state, half, rows, width, key_of(seed_dgate), key_of(seed_dup), key_of(seed_product), reinterpret_cast<const Key *>(seed_device),
                         d_gate, d_up, ld_dgate, ld_dup, d_gate_cells, d_up_cells, product_cells, across, count,
                         wide(gy, ld_gy, dtype), wide(d_gate, ld_dgate, dtype), wide(d_up, ld_dup, dtype)};
    pick_kernel(dtype, act, format, [&](auto dt, auto ac, auto fmt) {
        hipLaunchKernelGGL((backward_kernel<dt(), ac(), fmt()>), dim3(grid_of(count)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

}  // extern "C"
