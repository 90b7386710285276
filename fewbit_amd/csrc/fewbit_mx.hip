// fewbit_mx.hip -- a matrix kept as OCP-MX cells down its columns, and the weight gradient formed from two such buffers on the scaled matrix
// instruction of gfx950; part of the companion library libfewbit_hipx.so (include/fewbit_hipx.h, "The row blocks of a seed"; the definition:
// fewbit_mxdef.h):
//
//     mx_pack     rows x width (bf16 / fp16 / fp32, row stride ld) -> scales [blocks][width], codes [blocks][width][cell]      ONE launch
//     mx_unpack   the decode of such a buffer as a contiguous rows x width tensor                                                ONE launch
//     mx_wgrad    out[o][i] = sum_r G^[r][o] * X^[r][i],  G^ an fp8 buffer of rows x out_features, X^ an fp4 / fp6 buffer of rows x in_features,
//                 on v_mfma_scale_f32_32x32x64_f8f6f4: the code bytes go from memory into the operand registers as they lie, the E8M0 bytes
//                 into the instruction's scale operands.  Nothing is decoded.
//
// ---- mx_pack: a transpose (memory runs along rows, cells run down columns) -----------------------------------------------------------------------
//   workgroup  256 lanes take a tile of 32 rows (ONE block b) x 64 columns; the grid walks the tiles.
//   load       lane t: row t / 8, columns 8 (t % 8) .. + 7 of the tile: one 16-byte piece (two at fp32) where src and ld allow and the piece is
//              inside the matrix, element loads otherwise -- the same values either way.  Rows and columns outside count as +0.  -> LDS tile.
//   round      lane t: column t % 64, row octet t / 64 (wave-uniform): reads its eight values down the column (consecutive lanes, consecutive
//              words: no conflict), max of the magnitude bits (an unsigned integer max; non-finite <=> the max is >= 0x7f800000), four octets
//              meet through 1 KiB of LDS; one Philox call; eight codes in integer arithmetic (mx::code_of).  -> LDS image of the tile's cells.
//   store      the tile's cells are contiguous in the buffer (64 * cell bytes): 8-byte pieces, consecutive lanes consecutive pieces; the 64
//              scale bytes from the first wave.  No atomics, no workspace: the same arguments give the same bytes.
//   The hardware's v_cvt_scalef32_sr_* conversions are not used: their stochastic rounding adds the random bits below the kept mantissa of the
//   fp32 input, which is not the header's "cut the fraction to 16 bits" for elements far below the cell's amax; integers are bit for bit the host's.
// ---- mx_unpack: the same tile the other way round (cells -> LDS by 8-byte pieces, a lane decodes eight columns of one row) -------------------------
// ---- mx_wgrad (ONE plan for every served call; make_plan) -------------------------------------------------------------------------------------------
//   workgroup  4 waves own 128 out_features x 128 in_features: waves 2 (out) x 2 (in), each 64 x 64 = 2 x 2 blocks of the 32 x 32 x 64
//              instruction -> 64 fp32 accumulators per lane.
//   K step     64 rows = two row blocks, K block h = rows of block 2 s + h.  The SCALE operand of lane (c, h) is the scale byte of K block h of
//              column c (op_sel 0: byte 0 of the register).  The CODES of a 4- or 6-bit operand sit the same way: lane (c, h) holds the 32 K
//              values of block h, ONE cell -- one 16-byte load (fp4) or three 8-byte loads (fp6: cells are 24 bytes), neighbouring lanes
//              neighbouring cells (32 lanes: 512 bytes at fp4).  An 8-bit operand is laid out as the unscaled fp8 instructions have it, in
//              halves of 16: registers 0 .. 3 of lane (c, h) are K 16 h .. 16 h + 15, registers 4 .. 7 are K 32 + 16 h .. 32 + 16 h + 15
//              (established on the hardware with one-hot cells; the compiler and the ISA text leave it open).  So an A fragment is 16 bytes
//              from the cell of block 2 s and 16 from that of block 2 s + 1, at offset 16 h: the two half waves read the two halves of the
//              same cells.
//              Loads are plain global loads, software-pipelined one K step ahead in two register sets (no LDS, no barrier).
//   edges      a block at or beyond ceil(rows / 32), and a column block outside the matrix, are zero codes with scale byte 0 that are never
//              loaded.  Rows inside the last block but beyond `rows` were packed as +0.
//   poison     a poisoned fp8 cell holds the format's NaN in every code, so its products are NaN whatever the scale does; fp4 and fp6 have no
//              NaN, so the kernel itself ORs "scale byte == 0xFF" per lane (= per column of out) and the epilogue writes NaN there.
//   split K    gridDim.z slices of K steps when the tiles alone cannot fill 256 CUs: fp32 partial sums in the workspace, a second kernel adds
//              them in slice order and rounds once.  No atomics.  The slice count is capped so that the workspace stays within
//              rows * in_features * 2 bytes (a 16-bit decode of X^).
// Roofline class: MFMA (scaled f8f6f4); flops = 2 * rows * in_features * out_features.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fewbit_hipx.h"
#include "fewbit_mxdef.h"

#pragma clang fp contract(off)

namespace fewbit_hip {
namespace mx {

constexpr int kTileCols = 64, kThreads = 256;
constexpr size_t kMaxTiles = size_t{1} << 20;             // workgroups of pack / unpack; beyond that a workgroup walks on by the grid's width

struct Tiles { size_t across, count; };
inline Tiles tiles_of(size_t rows, size_t width) {
    const size_t across = (width + kTileCols - 1) / kTileCols;
    return Tiles{across, across * blocks_of(rows)};
}
inline unsigned grid_of(const Tiles &t) { return static_cast<unsigned>(t.count < kMaxTiles ? t.count : kMaxTiles); }

template <int DT, int FMT>
__global__ __launch_bounds__(kThreads) void pack_kernel(const void *__restrict__ src_, size_t rows, size_t width, size_t ld, bool vec, uint32_t domain, Key value,
                                                        const Key *device, size_t across, size_t count, uint8_t *__restrict__ out) {
    using T = typename Elem<DT>::type;
    constexpr size_t kCell = cell_bytes(FMT);
    __shared__ T tile[kCellRows][kTileCols];
    __shared__ uint32_t amax_s[kOctets][kTileCols];
    __shared__ uint64_t image[kTileCols * kCell / 8];
    const T *src = static_cast<const T *>(src_);
    Key key = value;
    if (device != nullptr) key = *device;
    uint8_t *codes = out + codes_offset(rows, width);
    const int t = threadIdx.x;
    const int lrow = t >> 3, lcol = 8 * (t & 7);          // the load role
    const int c = t & (kTileCols - 1), o = t >> 6;        // the rounding role: column c, row octet o
    for (size_t tl = blockIdx.x; tl < count; tl += gridDim.x) {
        const size_t b = tl / across, j0 = (tl % across) * kTileCols;
        const size_t r = kCellRows * b + lrow, col = j0 + lcol;
        T raw[kBlock];
        if (vec && r < rows && col + kBlock <= width) {
            load8<DT>(src + r * ld + col, raw);
        } else {
#pragma unroll
            for (int k = 0; k < kBlock; ++k) raw[k] = r < rows && col + k < width ? src[r * ld + col + k] : T{0};
        }
#pragma unroll
        for (int k = 0; k < kBlock; ++k) tile[lrow][lcol + k] = raw[k];
        __syncthreads();
        uint32_t v[kBlock], amax = 0;
#pragma unroll
        for (int k = 0; k < kBlock; ++k) {
            v[k] = widen<DT>(tile[kBlock * o + k][c]);
            const uint32_t m = v[k] & 0x7fffffffu;
            amax = m > amax ? m : amax;
        }
        amax_s[o][c] = amax;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kOctets; ++k) amax = amax_s[k][c] > amax ? amax_s[k][c] : amax;
        const bool bad = amax >= 0x7f800000u;
        const int e = bad ? 128 : scale_of_amax<FMT>(amax);
        uint32_t w[4];
        octet_words(b, j0 + c, width, o, domain, key, w);
        const uint64_t word = octet_codes<FMT>(v, e, bad, w);
        if constexpr (FMT == 4) reinterpret_cast<uint32_t *>(image)[kOctets * c + o] = static_cast<uint32_t>(word);
        else if constexpr (FMT == 8) image[kOctets * c + o] = word;
        else {
            uint16_t *at = reinterpret_cast<uint16_t *>(image) + 12 * c + 3 * o;
            at[0] = static_cast<uint16_t>(word), at[1] = static_cast<uint16_t>(word >> 16), at[2] = static_cast<uint16_t>(word >> 32);
        }
        if (o == 0 && j0 + c < width) out[b * width + j0 + c] = static_cast<uint8_t>(e + 127);
        __syncthreads();
        const size_t have = (width - j0 < static_cast<size_t>(kTileCols) ? width - j0 : kTileCols) * kCell;
        if (8 * static_cast<size_t>(t) < have) reinterpret_cast<uint64_t *>(codes + (b * width + j0) * kCell)[t] = image[t];
        // (the next round writes `tile` behind this round's second barrier's reads, `amax_s` and `image` behind its third: no barrier here)
    }
}

template <int DT, int FMT>
__global__ __launch_bounds__(kThreads) void unpack_kernel(const uint8_t *__restrict__ packed, size_t rows, size_t width, bool vec, size_t across, size_t count,
                                                          void *__restrict__ out_) {
    using T = typename Elem<DT>::type;
    constexpr size_t kCell = cell_bytes(FMT);
    __shared__ uint64_t image[kTileCols * kCell / 8];
    __shared__ uint8_t scale_s[kTileCols];
    T *out = static_cast<T *>(out_);
    const uint8_t *codes = packed + codes_offset(rows, width);
    const int t = threadIdx.x, lrow = t >> 3, lcol = 8 * (t & 7);
    for (size_t tl = blockIdx.x; tl < count; tl += gridDim.x) {
        const size_t b = tl / across, j0 = (tl % across) * kTileCols;
        const size_t cols = width - j0 < static_cast<size_t>(kTileCols) ? width - j0 : kTileCols;
        if (8 * static_cast<size_t>(t) < cols * kCell) image[t] = reinterpret_cast<const uint64_t *>(codes + (b * width + j0) * kCell)[t];
        if (static_cast<size_t>(t) < cols) scale_s[t] = packed[b * width + j0 + t];
        __syncthreads();
        const size_t r = kCellRows * b + lrow, col = j0 + lcol;
        const uint8_t *bytes = reinterpret_cast<const uint8_t *>(image);
        T y[kBlock];
#pragma unroll
        for (int k = 0; k < kBlock; ++k) {
            const size_t bit = kCell * 8 * (lcol + k) + FMT * lrow;
            uint32_t two = bytes[bit / 8];
            if (bit % 8 + FMT > 8) two |= static_cast<uint32_t>(bytes[bit / 8 + 1]) << 8;      // (fp6 only, and never for a cell's last code)
            const float value = lcol + k < static_cast<int>(cols) ? decode<FMT>((two >> (bit % 8)) & ((1u << FMT) - 1u), scale_s[lcol + k]) : 0.0f;
            y[k] = narrow<DT>(value);
        }
        if (r < rows) {
            if (vec && col + kBlock <= width) {
                store8<DT>(out + r * width + col, y);
            } else {
#pragma unroll
                for (int k = 0; k < kBlock; ++k)
                    if (col + k < width) out[r * width + col + k] = y[k];
            }
        }
        __syncthreads();
    }
}

// ---- the weight gradient ---------------------------------------------------------------------------------------------------------------------------
constexpr int BM = 128, BN = 128, BK = 64;
constexpr size_t kTargetGroups = 256;       // workgroups the plan tries to reach by slicing the rows (the CUs of an MI355X; the plan does not ask the device)
constexpr size_t kMaxWgradWidth = size_t{1} << 22;

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

struct Plan { size_t tiles_in, tiles_out, slices, per_slice; };   // per_slice: K steps (of BK rows) of a slice

inline bool serves(size_t rows, size_t in_features, size_t out_features, int format) {
    const size_t wider = in_features > out_features ? in_features : out_features;
    return (format == 4 || format == 6) && rows >= 1 && in_features >= 32 && out_features >= 32 && in_features % 32 == 0 && out_features % 32 == 0 &&
           wider <= kMaxWgradWidth && rows <= kMaxCount / wider && in_features * out_features <= kMaxCount;
}

inline Plan make_plan(size_t rows, size_t in_features, size_t out_features) {
    Plan p;
    p.tiles_in = (in_features + BN - 1) / BN;
    p.tiles_out = (out_features + BM - 1) / BM;
    const size_t steps = (rows + BK - 1) / BK, cap = rows / (2 * out_features);        // slices * out * in * 4 <= rows * in * 2
    size_t want = kTargetGroups / (p.tiles_in * p.tiles_out);
    want = want < cap ? want : cap;
    want = want < steps ? want : steps;
    want = want < 65535 ? want : 65535;
    if (want < 2) want = 1;
    p.per_slice = (steps + want - 1) / want;
    p.slices = (steps + p.per_slice - 1) / p.per_slice;                                 // (no empty slice)
    return p;
}

inline size_t workspace_of(const Plan &p, size_t in_features, size_t out_features) {
    return p.slices > 1 ? p.slices * out_features * in_features * sizeof(float) : 0;
}

// the operands of one K step in one lane: two cells of G^ (fp8: 8 dwords each) and two of X^ (FMT dwords each), and their scale bytes
struct Operands { i32x8 a[2], b[2]; int sa[2], sb[2]; };

// grid: x = tiles along in_features, y = tiles along out_features, z = K slices; `out_`: the result (ODT), or with several slices the workspace (ODT =
// FEWBIT_F32), where slice z writes its partial sums at z * out_features * in_features
template <int FMT, int ODT>
__global__ __launch_bounds__(kThreads) void wgrad_kernel(const uint8_t *__restrict__ g, const uint8_t *__restrict__ x, size_t rows, size_t in_features, size_t out_features,
                                                         size_t per_slice, void *__restrict__ out_) {
    constexpr size_t kCell = cell_bytes(FMT);
    constexpr int kBlgp = FMT == 4 ? 4 : 2;                                           // the instruction's name for E2M1 / E2M3 (E4M3: 0)
    const size_t blocks = blocks_of(rows), steps = (blocks + 1) / 2;
    const uint8_t *gcodes = g + codes_offset(rows, out_features), *xcodes = x + codes_offset(rows, in_features);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const size_t m0 = static_cast<size_t>(blockIdx.y) * BM + 64 * (wave & 1), n0 = static_cast<size_t>(blockIdx.x) * BN + 64 * (wave >> 1);
    const size_t begin = static_cast<size_t>(blockIdx.z) * per_slice;
    const size_t end = begin + per_slice < steps ? begin + per_slice : steps;
    if (begin >= end) return;                                                         // (block-uniform; cannot happen with the host's slicing)

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    uint32_t poisoned[2] = {0u, 0u};

    auto fetch = [&](size_t step, Operands &f) __attribute__((always_inline)) {
        const size_t kb = 2 * step + h;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const size_t col = m0 + 32 * i + c;
            f.a[i] = i32x8{0, 0, 0, 0, 0, 0, 0, 0};
            f.sa[i] = 0;
            if (col < out_features) {
                // (an 8-bit operand is two halves of 16 K values: registers 0 .. 3 are K 16 h .. 16 h + 15, registers 4 .. 7 are K 32 + 16 h .. -- rows
                // 16 h .. of block 2 s and of block 2 s + 1 -- while the lane's SCALE is that of K block h, whichever lanes hold its values)
                const size_t cell = 2 * step * out_features + col;                      // (block 2 s is inside: step < steps)
                const u32x4 lo = *reinterpret_cast<const u32x4 *>(gcodes + cell * 32 + 16 * h);
                u32x4 hi = u32x4{0u, 0u, 0u, 0u};
                if (2 * step + 1 < blocks) hi = *reinterpret_cast<const u32x4 *>(gcodes + (cell + out_features) * 32 + 16 * h);
                f.a[i] = i32x8{int(lo.x), int(lo.y), int(lo.z), int(lo.w), int(hi.x), int(hi.y), int(hi.z), int(hi.w)};
                if (kb < blocks) f.sa[i] = g[kb * out_features + col];
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const size_t col = n0 + 32 * j + c;
            f.b[j] = i32x8{0, 0, 0, 0, 0, 0, 0, 0};
            f.sb[j] = 0;
            if (kb < blocks && col < in_features) {
                const size_t cell = kb * in_features + col;
                if constexpr (FMT == 4) {
                    const u32x4 v = *reinterpret_cast<const u32x4 *>(xcodes + cell * kCell);
                    f.b[j] = i32x8{int(v.x), int(v.y), int(v.z), int(v.w), 0, 0, 0, 0};
                } else {
                    const u32x2 *p = reinterpret_cast<const u32x2 *>(xcodes + cell * kCell);
                    const u32x2 v0 = p[0], v1 = p[1], v2 = p[2];
                    f.b[j] = i32x8{int(v0.x), int(v0.y), int(v1.x), int(v1.y), int(v2.x), int(v2.y), 0, 0};
                }
                f.sb[j] = x[cell];
            }
        }
    };
    auto multiply = [&](const Operands &f) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 2; ++j) poisoned[j] |= f.sb[j] == static_cast<int>(kPoisonScale) ? 1u : 0u;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(f.a[i], f.b[j], acc[i][j], 0, kBlgp, 0, f.sa[i], 0, f.sb[j]);
    };

    // two register sets: the loads of step s + 1 go out in front of the MFMAs of step s
    Operands f0, f1;
    size_t s = begin;
    fetch(s, f0);
    for (;;) {
        if (s + 1 < end) fetch(s + 1, f1);
        multiply(f0);
        if (++s >= end) break;
        if (s + 1 < end) fetch(s + 1, f0);
        multiply(f1);
        if (++s >= end) break;
    }

    // ---- epilogue: accumulator register r of block (i, j) is out_feature m0 + 32 i + 8 (r / 4) + 4 h + r % 4, in_feature n0 + 32 j + c
    using T = typename Elem<ODT>::type;
    T *out = static_cast<T *>(out_) + static_cast<size_t>(blockIdx.z) * out_features * in_features;      // (one slice: z = 0)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const size_t col = n0 + 32 * j + c;
        const bool nan = (poisoned[j] | static_cast<uint32_t>(__shfl_xor(static_cast<int>(poisoned[j]), 32))) != 0;    // the column's other half of K
        if (col >= in_features) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const size_t o = m0 + 32 * i + 8 * (r >> 2) + 4 * h + (r & 3);
                if (o < out_features) out[o * in_features + col] = narrow<ODT>(nan ? float_of_bits(kNaN) : acc[i][j][r]);
            }
    }
}

// partial sums -> result, four elements per lane: a fixed order (slice 0, 1, 2, ...), one rounding
template <int ODT> __global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ ws, size_t n4, int slices, void *__restrict__ out) {
    const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n4) return;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(ws) + i;
    f32x4 s = src[0];
    for (int z = 1; z < slices; ++z) s += src[static_cast<size_t>(z) * n4];
    if constexpr (ODT == FEWBIT_F32) {
        reinterpret_cast<f32x4 *>(out)[i] = s;
    } else {
        u32x2 o;
        o.x = narrow<ODT>(s.x) | static_cast<uint32_t>(narrow<ODT>(s.y)) << 16;
        o.y = narrow<ODT>(s.z) | static_cast<uint32_t>(narrow<ODT>(s.w)) << 16;
        reinterpret_cast<u32x2 *>(out)[i] = o;
    }
}

// what the entry points that take a matrix refuse alike, the pointers last; 1: no elements, nothing to do
inline int check_matrix(const char *name, int format, size_t rows, size_t width, const void *from, const void *to) {
    if (const int rc = check_format(name, format)) return rc;
    if (rows == 0 || width == 0) return 1;
    if (width > kMaxWidth) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: width = %zu is beyond 2^23", name, width);
    if (rows > kMaxCount / width) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: rows * width = %zu * %zu is beyond 2^36", name, rows, width);
    return from == nullptr || to == nullptr ? refuse_null(name) : FEWBIT_OK;
}
inline int check_role(const char *name, int role) {
    return role == 0 || role == 1 ? FEWBIT_OK : fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: role = %d is not 0 (a kept input) or 1 (a gradient)", name, role);
}
inline int check_aligned16(const char *name, const char *what, const void *p) {
    return !misaligned(p, 16) ? FEWBIT_OK : fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: %s must be 16-byte aligned", name, what);
}

}  // namespace mx
}  // namespace fewbit_hip

using namespace fewbit_hip;

extern "C" {

size_t fewbit_hipx_mx_bytes(size_t rows, size_t width, int format) { return mx::bytes_of(rows, width, format); }

int fewbit_hipx_mx_pack_host(const float *x_host, size_t rows, size_t width, int format, int role, uint64_t seed, uint8_t *out_host) {
    using namespace mx;
    const char *name = "mx_pack_host";
    if (const int rc = check_role(name, role)) return rc;
    if (const int rc = check_matrix(name, format, rows, width, x_host, out_host)) return rc < 0 ? rc : FEWBIT_OK;
    const Key key = sketch::key_of(seed);
    const uint32_t domain = domain_of(role);
    uint8_t *codes = out_host + codes_offset(rows, width);
    for (size_t i = blocks_of(rows) * width; i < codes_offset(rows, width); ++i) out_host[i] = 0;        // (the gap in front of the codes: written here, not by the kernel)
    pick_format(format, [&](auto fmt) {
        for (size_t b = 0; b < blocks_of(rows); ++b) {
            const size_t have = rows - kCellRows * b < static_cast<size_t>(kCellRows) ? rows - kCellRows * b : kCellRows;
            for (size_t j = 0; j < width; ++j)
                pack_cell_host<fmt()>(x_host + kCellRows * b * width + j, width, have, b, j, width, domain, key, out_host + b * width + j,
                                      codes + (b * width + j) * cell_bytes(fmt()));
        }
    });
    return FEWBIT_OK;
}

int fewbit_hipx_mx_unpack_host(const uint8_t *packed_host, size_t rows, size_t width, int format, float *out_host) {
    using namespace mx;
    if (const int rc = check_matrix("mx_unpack_host", format, rows, width, packed_host, out_host)) return rc < 0 ? rc : FEWBIT_OK;
    const uint8_t *codes = packed_host + codes_offset(rows, width);
    pick_format(format, [&](auto fmt) {
        for (size_t r = 0; r < rows; ++r)
            for (size_t j = 0; j < width; ++j) {
                const size_t cell = r / kCellRows * width + j;
                out_host[r * width + j] = decode_cell_host<fmt()>(codes + cell * cell_bytes(fmt()), packed_host[cell], r % kCellRows);
            }
    });
    return FEWBIT_OK;
}

int fewbit_hipx_mx_pack(int dtype, const void *src, size_t rows, size_t width, size_t ld, int format, int role, uint64_t seed, const uint64_t *seed_device,
                        uint8_t *out, size_t out_bytes, void *stream) {
    using namespace mx;
    const char *name = "mx_pack";
    if (const int rc = check_dtype(name, dtype)) return rc;
    if (const int rc = check_role(name, role)) return rc;
    if (const int rc = check_seed_word(name, seed_device)) return rc;
    if (const int rc = check_matrix(name, format, rows, width, src, out)) return rc < 0 ? rc : FEWBIT_OK;
    if (ld < width) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: ld = %zu must be at least width = %zu", name, ld, width);
    if (misaligned(src, size_of(dtype))) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: src must be aligned to its element size", name);
    if (const int rc = check_aligned16(name, "out", out)) return rc;
    if (const int rc = check_bytes(name, "out", out_bytes, bytes_of(rows, width, format))) return rc;
    const Tiles tiles = tiles_of(rows, width);
    const bool vec = !misaligned(src, 16) && ld * size_of(dtype) % 16 == 0;
    const Key key = sketch::key_of(seed);
    pick_dtype(dtype, [&](auto dt) {
        pick_format(format, [&](auto fmt) {
            hipLaunchKernelGGL((pack_kernel<dt(), fmt()>), dim3(grid_of(tiles)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), src, rows, width, ld, vec,
                               domain_of(role), key, reinterpret_cast<const Key *>(seed_device), tiles.across, tiles.count, out);
        });
    });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

int fewbit_hipx_mx_unpack(const uint8_t *packed, size_t packed_bytes, size_t rows, size_t width, int format, int out_dtype, void *out, void *stream) {
    using namespace mx;
    const char *name = "mx_unpack";
    if (const int rc = check_dtype(name, out_dtype)) return rc;
    if (const int rc = check_matrix(name, format, rows, width, packed, out)) return rc < 0 ? rc : FEWBIT_OK;
    if (const int rc = check_aligned16(name, "packed", packed)) return rc;
    if (misaligned(out, size_of(out_dtype))) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: out must be aligned to its element size", name);
    if (const int rc = check_bytes(name, "packed", packed_bytes, bytes_of(rows, width, format))) return rc;
    const Tiles tiles = tiles_of(rows, width);
    const bool vec = !misaligned(out, 16) && width * size_of(out_dtype) % 16 == 0;
    pick_dtype(out_dtype, [&](auto dt) {
        pick_format(format, [&](auto fmt) {
            hipLaunchKernelGGL((unpack_kernel<dt(), fmt()>), dim3(grid_of(tiles)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), packed, rows, width, vec,
                               tiles.across, tiles.count, out);
        });
    });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

size_t fewbit_hipx_mx_wgrad_workspace(size_t rows, size_t in_features, size_t out_features, int format) {
    using namespace mx;
    if (!serves(rows, in_features, out_features, format)) return 0;
    return workspace_of(make_plan(rows, in_features, out_features), in_features, out_features);
}

int fewbit_hipx_mx_wgrad(const uint8_t *grad, size_t grad_bytes, const uint8_t *kept, size_t kept_bytes, int format, size_t rows, size_t in_features,
                         size_t out_features, int out_dtype, void *out, void *workspace, size_t workspace_bytes, void *stream) {
    using namespace mx;
    const char *name = "mx_wgrad";
    if (const int rc = check_dtype(name, out_dtype)) return rc;
    if (const int rc = check_format(name, format)) return rc;
    if (rows == 0) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: rows = 0", name);
    if (!serves(rows, in_features, out_features, format))
        return fail(FEWBIT_ERR_UNSUPPORTED, "%s: format = %d, rows = %zu, in_features = %zu, out_features = %zu has no kernel (fp4 or fp6 kept; both widths multiples of 32 up to %zu)",
                    name, format, rows, in_features, out_features, kMaxWgradWidth);
    if (grad == nullptr || kept == nullptr || out == nullptr) return refuse_null(name);
    if (const int rc = check_aligned16(name, "grad", grad)) return rc;
    if (const int rc = check_aligned16(name, "kept", kept)) return rc;
    if (const int rc = check_aligned16(name, "out", out)) return rc;
    if (const int rc = check_bytes(name, "grad", grad_bytes, bytes_of(rows, out_features, 8))) return rc;
    if (const int rc = check_bytes(name, "kept", kept_bytes, bytes_of(rows, in_features, format))) return rc;
    const Plan plan = make_plan(rows, in_features, out_features);
    const size_t need = workspace_of(plan, in_features, out_features);
    if (need != 0) {
        if (workspace == nullptr) return refuse_null(name);
        if (const int rc = check_aligned16(name, "the workspace", workspace)) return rc;
        if (const int rc = check_bytes(name, "the workspace", workspace_bytes, need)) return rc;
    }
    const bool sliced = plan.slices > 1;
    const dim3 grid(static_cast<unsigned>(plan.tiles_in), static_cast<unsigned>(plan.tiles_out), static_cast<unsigned>(plan.slices));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (a sliced call: the product kernel writes fp32 partial sums into the workspace, the second kernel the result)
    pick<4, 6>(format, [&](auto fmt) {
        pick_dtype(sliced ? FEWBIT_F32 : out_dtype, [&](auto dt) {
            hipLaunchKernelGGL((wgrad_kernel<fmt(), dt()>), grid, dim3(kThreads), 0, s, grad, kept, rows, in_features, out_features, plan.per_slice, sliced ? workspace : out);
        });
    });
    if (sliced) {
        const size_t n4 = out_features * in_features / 4;
        pick_dtype(out_dtype, [&](auto dt) {
            hipLaunchKernelGGL((wgrad_reduce_kernel<dt()>), dim3(static_cast<unsigned>((n4 + 255) / 256)), dim3(256), 0, s, static_cast<const float *>(workspace), n4,
                               static_cast<int>(plan.slices), out);
        });
    }
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

}  // extern "C"
