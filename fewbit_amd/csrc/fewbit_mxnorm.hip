// fewbit_mxnorm.hip -- the RMS norm in front of linear layers that keep their input as OCP-MX cells: the norm keeps its normalized rows x^ as ONE
// mx_pack buffer and one fp32 rstd per row, which serve its own backward and, because y = x^ * gamma, every weight gradient behind it
// (dW = (G^T x^) * gamma by columns, mx_wgrad on the cells as they lie), on gfx950; part of the companion library libfewbit_hipx.so
// (include/fewbit_hipx.h, "The normalized rows as row blocks"):
//
//     mx_rms_norm_forward    x, gamma -> y, rstd and the cells of the FP32 x^ = x * rstd                                               ONE launch
//     mx_rms_norm_backward   gy, the cells, rstd, gamma -> dx, and the workgroups' column sums of gy * x^q -> dgamma      ONE launch and a small one
//
// The format is fewbit_mxdef.h's (scale_of_amax, octet_words, octet_codes, decode, used as they are); the formulas are those of fewbit_norm.hip's RMS
// kind.  What is new is the walk.  The norm kernels hold a row in the registers of one row of lanes; a cell needs 32 rows of a column together.  So:
//   workgroup  1024 lanes own ONE row block b (32 rows) and walk on by the grid's width.  Ownership of whole row blocks is what lets one kernel
//              know a row's statistic before it rounds the row, with no flag or atomic between workgroups.
//   forward A  wave w takes rows w and w + 16 of the block: a lane sums the squares of its 8-element pieces (piece l, l + 64, ..) in index order,
//              then the DPP / readlane order of norm::row_sum<64>.  rstd -> LDS and the output.
//   forward B  the block's 32 x 64 tiles, FOUR in flight, each on its own group of 256 lanes, with the two roles of mx::pack_kernel:
//              load role   lane u: row u / 8, columns 8 (u % 8) .. + 7: x again (from L2 by now: 32 * width * itemsize <= 512 KiB a workgroup),
//                          x^ = x * rstd, y = round(x^ * gamma) stored, the fp32 x^ into the group's LDS tile.
//              round role  lane u: column u % 64, row octet u / 64 (wave-uniform): eight values down the column, the four octets' amax meet
//                          through LDS, one Philox call, eight codes -> the LDS image of the cells.
//              store       whole cells in 8-byte pieces, consecutive lanes consecutive pieces; the scale bytes from the first wave of a group.
//              3 barriers a round of four tiles.  x is NOT held in LDS between the phases at any width: ONE plan, no thresholds
//              (cabi_x.MX_NORM_PLAN_WIDTHS is empty).  32 rows fit 160 KiB of LDS only up to 1280 elements of fp32; a block that small is read the
//              second time from L2 anyway, and the LDS it would take costs the second workgroup of a compute unit.
//   backward A (only where dx is wanted) the tiles in the same groups: cell images and scale bytes come into LDS by 8-byte pieces, alternating
//              between two images so that ONE barrier a round suffices; the lane decodes its eight x^q (mxglu's code_at + mx::decode), loads gy and
//              gamma and adds g^ x^q to its row's partial sum in index order.  The partial sums of a row meet in a fixed order: the eight lanes by
//              DPP (^1, ^2, the other quad), then the four groups in ascending order through LDS.  c = sum / width.
//   backward B the tiles again: dx = round(rstd * (g^ - x^q c)) stored; gy * x^q -> the group's LDS tile, whose 32 rows one wave adds in ascending
//              row order into the workgroup's row of the workspace [workgroups][width] (the same lane owns a column at every row block the
//              workgroup walks: a plain read-add-write of its own).  2 barriers a round.
//   column sums  a second launch adds the workgroups' rows in ascending order, associated by sixteenths -> dgamma.  At most kMaxGridBackward workgroups.
// Rows beyond `rows` count as +0 (their rstd is taken as 0), columns beyond `width` are neither rounded into a stored cell nor stored.
// Roofline class: memory (forward reads x once from memory and once from L2, writes y and 0.27 / 0.39 of it in cells).
//
// The sum of a seed in front of it (include/fewbit_hipx.h, "The sum of a seed in front of the normalized rows"): h = residual + dropout(x) normalized
// in the same launch, and the gradients of both behind the norm's backward:
//
//     mx_add_rms_norm_forward    x, residual, gamma -> y, rstd, the cells of h * rstd and, where asked for, h                             ONE launch
//     mx_add_rms_norm_backward   gy, [gh], the cells, rstd, gamma -> dres, dbranch, and the column sums -> dgamma         ONE launch and a small one
//
// Two kernels of their own (add_forward_kernel, add_backward_kernel) beside the plain pair, whose text and code stay as they were; the walk, the
// roles, the barriers and every sum's order are the plain kernels', so that every output is bit for bit fewbit_hipx_dropout with the residual as
// addend followed by the plain entry point.  What the fusion had to settle:
//   h twice    phase A forms h = narrow(x scale + residual) (fewbit_dropout.hip's `one` on widen / narrow) to sum the squares of the ROUNDED h, and
//              phase B RECOMPUTES it from x, the residual and the mask -- both inputs come from L2 by then, and the mask is a second Philox call per
//              eight elements.  h is written (phase A, where h_out is given) but never read back: post-norm it does not exist in memory, and there
//              is no workspace of the tokens' size.
//   one plan   with h_out phase B could load the stored h (one 16-byte load a piece, not two, and no second mask).  It does not: ONE plan at
//              every width and with or without h_out (cabi_x.MX_NORM_PLAN_WIDTHS stays empty), no read of a line another wave of the workgroup has
//              just written, and the pre-norm and the post-norm call have the same y, rstd and cells by construction and not by a second route.
//   the mask   is drawn on blocks of eight FLAT elements; with width % 8 == 0 the lane's piece in the load role (row r, columns col .. col + 7) is
//              flat block (r width + col) / 8 exactly, in phase A's walk (piece l, l + 64, ..) and in phase B's alike: one draw per lane and
//              piece, no LDS traffic.  threshold = 0 draws nothing and serves every width; a mask at another width is refused.
//   backward   phase A is the plain one.  Phase B rounds dx as the plain kernel does, adds gh as torch adds two tensors (both widened, the fp32 sum
//              rounded once) -> dres, and draws the piece's mask once more for dbranch = keep ? narrow(dres scale) : +0: one 16-byte load and one
//              16-byte store a piece more than the plain kernel.  With threshold = 0 dbranch is dres and must be absent.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fewbit_hipx.h"
#include "fewbit_mxdef.h"
#include "fewbit_mxrows.h"

#pragma clang fp contract(off)

namespace fewbit_hip {
namespace quant {
namespace mxnorm {

using namespace mxrows;            // the geometry, the lane sums, the two roles of a tile and the refusals: fewbit_mxrows.h

inline size_t workspace_of(size_t rows, size_t width) { return known_shape(rows, width) ? backward_grid(rows) * width * sizeof(float) : 0; }

struct ForwardArgs {
    const void *x;
    size_t ld_x, rows, width;
    const void *gamma;
    float eps;
    Key key;
    const Key *device;                      // nullptr, or the key in device memory
    void *y;
    size_t ld_y;
    float *rstd;
    uint8_t *cells;
    size_t blocks;
    bool vec_x, vec_y, vec_gamma;
};
struct BackwardArgs {
    const void *gy;
    size_t ld_gy;
    const uint8_t *cells;
    const float *rstd;
    const void *gamma;
    size_t rows, width;
    void *dx;                               // may be absent, and so may partials: what is absent is not written
    size_t ld_dx;
    float *partials;
    size_t blocks;
    bool vec_gy, vec_dx, vec_gamma;
};

template <int DT, int FMT>
__global__ __launch_bounds__(kThreads) void forward_kernel(ForwardArgs a) {
    using T = typename Elem<DT>::type;
    constexpr size_t kCell = mx::cell_bytes(FMT);
    __shared__ float rstd_s[kRows];
    __shared__ uint32_t tile[kGroups][kRows][kTileCols];                        // the fp32 bits of x^
    __shared__ uint32_t amax_s[kGroups][kOctets][kTileCols];
    __shared__ uint64_t image[kGroups][kTileCols * kCell / 8];
    const T *x = static_cast<const T *>(a.x), *gamma = static_cast<const T *>(a.gamma);
    T *y = static_cast<T *>(a.y);
    Key key = a.key;
    if (a.device != nullptr) key = *a.device;
    const size_t rows = a.rows, width = a.width;
    uint8_t *codes = a.cells + mx::codes_offset(rows, width);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int grp = t >> 8, u = t & (kGroupThreads - 1);
    const int lrow = u >> 3, lcol = 8 * (u & 7);          // the load role
    const int c = u & (kTileCols - 1), o = u >> 6;        // the rounding role: column c, row octet o
    const size_t across = (width + kTileCols - 1) / kTileCols, rounds = (across + kGroups - 1) / kGroups, pieces = (width + kBlock - 1) / kBlock;
    const float count = static_cast<float>(width);
    for (size_t b = blockIdx.x; b < a.blocks; b += gridDim.x) {
        // ---- phase A: the statistic of the block's rows, a wave per row ----
        for (int lr = wave; lr < kRows; lr += kWaves) {
            const size_t r = kRows * b + lr;
            float s = 0.0f;
            if (r < rows) {
                for (size_t p = lane; p < pieces; p += 64) {
                    T raw[kBlock];
                    load_piece<DT>(x, a.ld_x, a.vec_x, r, kBlock * p, rows, width, raw);
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) {
                        const float v = float_of_bits(widen<DT>(raw[k]));
                        s = add_rn(s, mul_rn(v, v));                            // (a missing element: +0)
                    }
                }
            }
            s = wave_sum(s);
            const float rstd = div_rn(1.0f, sqrt_rn(add_rn(div_rn(s, count), a.eps)));
            if (lane == 0) {
                rstd_s[lr] = r < rows ? rstd : 0.0f;
                if (r < rows) a.rstd[r] = rstd;
            }
        }
        __syncthreads();
        // ---- phase B: the block's tiles, four in flight ----
        for (size_t round = 0; round < rounds; ++round) {
            const size_t tl = round * kGroups + grp, j0 = tl * kTileCols;
            const bool have = tl < across;                                      // (the same for every lane of a group; the barriers are outside)
            const size_t cols = !have ? 0 : width - j0 < static_cast<size_t>(kTileCols) ? width - j0 : kTileCols;
            if (have) {
                const size_t r = kRows * b + lrow, col = j0 + lcol;
                T rx[kBlock], rg[kBlock], ry[kBlock];
                load_piece<DT>(x, a.ld_x, a.vec_x, r, col, rows, width, rx);
                load_piece<DT>(gamma, 0, a.vec_gamma, 0, col, 1, width, rg);
                const float rstd = rstd_s[lrow];
#pragma unroll
                for (int k = 0; k < kBlock; ++k) {
                    const float xhat = mul_rn(float_of_bits(widen<DT>(rx[k])), rstd);
                    ry[k] = narrow<DT>(mul_rn(xhat, float_of_bits(widen<DT>(rg[k]))));
                    tile[grp][lrow][lcol + k] = bits_of_float(xhat);
                }
                store_piece<DT>(y, a.ld_y, a.vec_y, r, col, rows, width, ry);
            }
            __syncthreads();
            uint32_t v[kBlock];
            if (have) column_amax(tile[grp], c, o, v, amax_s[grp]);
            __syncthreads();
            if (have) column_codes<FMT>(v, amax_s[grp], c, o, b, j0 + c, width, key, image[grp], a.cells);
            __syncthreads();
            store_cells<FMT>(image[grp], codes, b, j0, width, cols, u);
            // (the next round writes `tile` behind this round's second barrier's reads, `amax_s` and `image` behind its third, and the next block
            // writes rstd_s behind the reads in front of this round's first: no barrier here)
        }
    }
}

template <int DT, int FMT>
__global__ __launch_bounds__(kThreads) void backward_kernel(BackwardArgs a) {
    using T = typename Elem<DT>::type;
    constexpr size_t kCell = mx::cell_bytes(FMT);
    __shared__ uint64_t image[2][kGroups][kTileCols * kCell / 8];
    __shared__ uint8_t scale_s[2][kGroups][kTileCols];
    __shared__ float tile[kGroups][kRows][kTileCols];                           // gy * x^q
    __shared__ float part_s[kGroups][kRows], c_s[kRows];
    const T *gy = static_cast<const T *>(a.gy), *gamma = static_cast<const T *>(a.gamma);
    T *dx = static_cast<T *>(a.dx);
    const size_t rows = a.rows, width = a.width;
    const uint8_t *codes = a.cells + mx::codes_offset(rows, width);
    float *mine = a.partials != nullptr ? a.partials + static_cast<size_t>(blockIdx.x) * width : nullptr;
    const int t = threadIdx.x;
    const int grp = t >> 8, u = t & (kGroupThreads - 1);
    const int lrow = u >> 3, lcol = 8 * (u & 7);          // the load role
    const size_t across = (width + kTileCols - 1) / kTileCols, rounds = (across + kGroups - 1) / kGroups;
    const float count = static_cast<float>(width);
    // the eight x^q, gy and g^ of the lane's piece of tile (b, j0) from the LDS image `par`
    auto piece = [&](int par, size_t b, size_t j0, size_t cols, float (&xq)[kBlock], float (&up)[kBlock], float (&gh)[kBlock]) {
        const size_t r = kRows * b + lrow, col = j0 + lcol;
        T rgy[kBlock], rg[kBlock];
        load_piece<DT>(gy, a.ld_gy, a.vec_gy, r, col, rows, width, rgy);
        load_piece<DT>(gamma, 0, a.vec_gamma, 0, col, 1, width, rg);
#pragma unroll
        for (int k = 0; k < kBlock; ++k) {
            const bool inside = r < rows && lcol + k < static_cast<int>(cols);
            xq[k] = inside ? mx::decode<FMT>(code_at<FMT>(image[par][grp], lcol + k, lrow), scale_s[par][grp][lcol + k]) : 0.0f;
            up[k] = float_of_bits(widen<DT>(rgy[k]));                           // (outside: +0)
            gh[k] = mul_rn(up[k], float_of_bits(widen<DT>(rg[k])));
        }
    };
    bool first = true;                                                          // of this workgroup's row blocks: its row of the workspace is written, not added to
    for (size_t b = blockIdx.x; b < a.blocks; b += gridDim.x, first = false) {
        if (dx != nullptr) {
            // ---- phase A: c = sum_j(g^ x^q) / width of the block's rows ----
            float s = 0.0f;
            for (size_t round = 0; round < rounds; ++round) {
                const size_t tl = round * kGroups + grp, j0 = tl * kTileCols;
                const bool have = tl < across;
                const size_t cols = !have ? 0 : width - j0 < static_cast<size_t>(kTileCols) ? width - j0 : kTileCols;
                const int par = static_cast<int>(round & 1);
                load_cells<FMT>(image[par][grp], codes, b, j0, width, cols, u);
                if (static_cast<size_t>(u) < cols) scale_s[par][grp][u] = a.cells[b * width + j0 + u];
                __syncthreads();                       // (round i + 1 writes the other image, last read in round i - 1: in front of this barrier)
                if (have) {
                    float xq[kBlock], up[kBlock], gh[kBlock];
                    piece(par, b, j0, cols, xq, up, gh);
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) s = add_rn(s, mul_rn(gh[k], xq[k]));
                }
            }
            s = eight_sum(s);
            if ((u & 7) == 0) part_s[grp][lrow] = s;
            __syncthreads();
            if (t < kRows) c_s[t] = div_rn(add_rn(add_rn(add_rn(part_s[0][t], part_s[1][t]), part_s[2][t]), part_s[3][t]), count);
            __syncthreads();
        }
        // ---- phase B: dx, and the column sums of gy * x^q down the block ----
        const size_t r = kRows * b + lrow;
        const float rstd = dx != nullptr && r < rows ? a.rstd[r] : 0.0f, cr = dx != nullptr ? c_s[lrow] : 0.0f;
        for (size_t round = 0; round < rounds; ++round) {
            const size_t tl = round * kGroups + grp, j0 = tl * kTileCols;
            const bool have = tl < across;
            const size_t cols = !have ? 0 : width - j0 < static_cast<size_t>(kTileCols) ? width - j0 : kTileCols;
            load_cells<FMT>(image[0][grp], codes, b, j0, width, cols, u);
            if (static_cast<size_t>(u) < cols) scale_s[0][grp][u] = a.cells[b * width + j0 + u];
            __syncthreads();
            if (have) {
                float xq[kBlock], up[kBlock], gh[kBlock];
                piece(0, b, j0, cols, xq, up, gh);
                if (dx != nullptr) {
                    T rdx[kBlock];
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) rdx[k] = narrow<DT>(mul_rn(rstd, sub_rn(gh[k], mul_rn(xq[k], cr))));
                    store_piece<DT>(dx, a.ld_dx, a.vec_dx, r, j0 + lcol, rows, width, rdx);
                }
                if (mine != nullptr) {
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) tile[grp][lrow][lcol + k] = mul_rn(up[k], xq[k]);
                }
            }
            __syncthreads();
            if (mine != nullptr && u < kTileCols && static_cast<size_t>(u) < cols) {
                float sum = tile[grp][0][u];
#pragma unroll 8
                for (int k = 1; k < kRows; ++k) sum = add_rn(sum, tile[grp][k][u]);
                mine[j0 + u] = first ? sum : add_rn(mine[j0 + u], sum);
            }
            // (the next round writes the image behind this round's second barrier, and `tile` behind its own first: no barrier here)
        }
    }
}

// dgamma[c] = the workgroups' sums of column c: the rows of the workspace in ascending order, associated by sixteenths (mxrows::add_partials)
__global__ __launch_bounds__(kThreads) void column_sums_kernel(const float *__restrict__ partials, size_t parts, size_t width, float *__restrict__ dgamma) {
    __shared__ float waves[kWaves][kTileCols];
    add_partials(partials, parts, width, width, blockIdx.x, dgamma, waves);
}

// ---- the sum of a seed in front of the norm: h = residual + dropout(x), and the gradients of the two behind the norm's backward -------------------
struct AddForwardArgs {
    const void *x, *residual;
    size_t ld_x, ld_res, rows, width;
    const void *gamma;
    float eps;
    Key key, mask_key;
    const Key *device;                      // nullptr, or the two keys in device memory: the cells', then the mask's
    uint32_t threshold;
    float scale;
    void *y, *h;                            // h may be absent: it is then not written
    size_t ld_y, ld_h;
    float *rstd;
    uint8_t *cells;
    size_t blocks;
    bool vec_x, vec_res, vec_y, vec_h, vec_gamma;
};
struct AddBackwardArgs {
    const void *gy, *gh;                    // gh may be absent: nothing is added
    size_t ld_gy, ld_gh;
    const uint8_t *cells;
    const float *rstd;
    const void *gamma;
    size_t rows, width;
    Key mask_key;
    const Key *device;                      // nullptr, or the mask's key in device memory
    uint32_t threshold;
    float scale;
    void *dres, *dbranch;                   // may each be absent, and so may partials: what is absent is not written
    size_t ld_dres, ld_dbranch;
    float *partials;
    size_t blocks;
    bool vec_gy, vec_gh, vec_dres, vec_dbranch, vec_gamma;
};

// (piece_mask, dropped_sum, dropped_gradient and sum_piece: fewbit_mxrows.h, shared with the layer norm's fused pair)

// forward_kernel with h = residual + dropout(x) in the place of x: formed in phase A (and stored where h is wanted), formed AGAIN in phase B
template <int DT, int FMT>
__global__ __launch_bounds__(kThreads) void add_forward_kernel(AddForwardArgs a) {
    using T = typename Elem<DT>::type;
    constexpr size_t kCell = mx::cell_bytes(FMT);
    __shared__ float rstd_s[kRows];
    __shared__ uint32_t tile[kGroups][kRows][kTileCols];                        // the fp32 bits of h^ = h * rstd
    __shared__ uint32_t amax_s[kGroups][kOctets][kTileCols];
    __shared__ uint64_t image[kGroups][kTileCols * kCell / 8];
    const T *gamma = static_cast<const T *>(a.gamma);
    T *y = static_cast<T *>(a.y), *h_out = static_cast<T *>(a.h);
    Key key = a.key, mask_key = a.mask_key;
    if (a.device != nullptr) key = a.device[0], mask_key = a.device[1];
    const size_t rows = a.rows, width = a.width;
    uint8_t *codes = a.cells + mx::codes_offset(rows, width);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int grp = t >> 8, u = t & (kGroupThreads - 1);
    const int lrow = u >> 3, lcol = 8 * (u & 7);          // the load role
    const int c = u & (kTileCols - 1), o = u >> 6;        // the rounding role: column c, row octet o
    const size_t across = (width + kTileCols - 1) / kTileCols, rounds = (across + kGroups - 1) / kGroups, pieces = (width + kBlock - 1) / kBlock;
    const float count = static_cast<float>(width);
    for (size_t b = blockIdx.x; b < a.blocks; b += gridDim.x) {
        // ---- phase A: h and the statistic of the block's rows, a wave per row ----
        for (int lr = wave; lr < kRows; lr += kWaves) {
            const size_t r = kRows * b + lr;
            float s = 0.0f;
            if (r < rows) {
                for (size_t p = lane; p < pieces; p += 64) {
                    T rh[kBlock];
                    sum_piece<DT>(a, mask_key, r, kBlock * p, rh);
                    if (h_out != nullptr) store_piece<DT>(h_out, a.ld_h, a.vec_h, r, kBlock * p, rows, width, rh);
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) {
                        const float v = float_of_bits(widen<DT>(rh[k]));
                        s = add_rn(s, mul_rn(v, v));                            // (a missing element: +0)
                    }
                }
            }
            s = wave_sum(s);
            const float rstd = div_rn(1.0f, sqrt_rn(add_rn(div_rn(s, count), a.eps)));
            if (lane == 0) {
                rstd_s[lr] = r < rows ? rstd : 0.0f;
                if (r < rows) a.rstd[r] = rstd;
            }
        }
        __syncthreads();
        // ---- phase B: the block's tiles, four in flight ----
        for (size_t round = 0; round < rounds; ++round) {
            const size_t tl = round * kGroups + grp, j0 = tl * kTileCols;
            const bool have = tl < across;                                      // (the same for every lane of a group; the barriers are outside)
            const size_t cols = !have ? 0 : width - j0 < static_cast<size_t>(kTileCols) ? width - j0 : kTileCols;
            if (have) {
                const size_t r = kRows * b + lrow, col = j0 + lcol;
                T rh[kBlock], rg[kBlock], ry[kBlock];
                sum_piece<DT>(a, mask_key, r, col, rh);
                load_piece<DT>(gamma, 0, a.vec_gamma, 0, col, 1, width, rg);
                const float rstd = rstd_s[lrow];
#pragma unroll
                for (int k = 0; k < kBlock; ++k) {
                    const float xhat = mul_rn(float_of_bits(widen<DT>(rh[k])), rstd);
                    ry[k] = narrow<DT>(mul_rn(xhat, float_of_bits(widen<DT>(rg[k]))));
                    tile[grp][lrow][lcol + k] = bits_of_float(xhat);
                }
                store_piece<DT>(y, a.ld_y, a.vec_y, r, col, rows, width, ry);
            }
            __syncthreads();
            uint32_t v[kBlock];
            if (have) column_amax(tile[grp], c, o, v, amax_s[grp]);
            __syncthreads();
            if (have) column_codes<FMT>(v, amax_s[grp], c, o, b, j0 + c, width, key, image[grp], a.cells);
            __syncthreads();
            store_cells<FMT>(image[grp], codes, b, j0, width, cols, u);
            // (no barrier here: forward_kernel)
        }
    }
}

// backward_kernel with dres = dx + gh and dbranch = the dropout's gradient of dres in the place of dx
template <int DT, int FMT>
__global__ __launch_bounds__(kThreads) void add_backward_kernel(AddBackwardArgs a) {
    using T = typename Elem<DT>::type;
    constexpr size_t kCell = mx::cell_bytes(FMT);
    __shared__ uint64_t image[2][kGroups][kTileCols * kCell / 8];
    __shared__ uint8_t scale_s[2][kGroups][kTileCols];
    __shared__ float tile[kGroups][kRows][kTileCols];                           // gy * x^q
    __shared__ float part_s[kGroups][kRows], c_s[kRows];
    const T *gy = static_cast<const T *>(a.gy), *gh = static_cast<const T *>(a.gh), *gamma = static_cast<const T *>(a.gamma);
    T *dres = static_cast<T *>(a.dres), *dbranch = static_cast<T *>(a.dbranch);
    Key mask_key = a.mask_key;
    if (a.device != nullptr) mask_key = *a.device;
    const bool wanted = dres != nullptr || dbranch != nullptr;
    const size_t rows = a.rows, width = a.width;
    const uint8_t *codes = a.cells + mx::codes_offset(rows, width);
    float *mine = a.partials != nullptr ? a.partials + static_cast<size_t>(blockIdx.x) * width : nullptr;
    const int t = threadIdx.x;
    const int grp = t >> 8, u = t & (kGroupThreads - 1);
    const int lrow = u >> 3, lcol = 8 * (u & 7);          // the load role
    const size_t across = (width + kTileCols - 1) / kTileCols, rounds = (across + kGroups - 1) / kGroups;
    const float count = static_cast<float>(width);
    // the eight x^q, gy and g^ of the lane's piece of tile (b, j0) from the LDS image `par`
    auto piece = [&](int par, size_t b, size_t j0, size_t cols, float (&xq)[kBlock], float (&up)[kBlock], float (&ghat)[kBlock]) {
        const size_t r = kRows * b + lrow, col = j0 + lcol;
        T rgy[kBlock], rg[kBlock];
        load_piece<DT>(gy, a.ld_gy, a.vec_gy, r, col, rows, width, rgy);
        load_piece<DT>(gamma, 0, a.vec_gamma, 0, col, 1, width, rg);
#pragma unroll
        for (int k = 0; k < kBlock; ++k) {
            const bool inside = r < rows && lcol + k < static_cast<int>(cols);
            xq[k] = inside ? mx::decode<FMT>(code_at<FMT>(image[par][grp], lcol + k, lrow), scale_s[par][grp][lcol + k]) : 0.0f;
            up[k] = float_of_bits(widen<DT>(rgy[k]));                           // (outside: +0)
            ghat[k] = mul_rn(up[k], float_of_bits(widen<DT>(rg[k])));
        }
    };
    bool first = true;                                                          // of this workgroup's row blocks: its row of the workspace is written, not added to
    for (size_t b = blockIdx.x; b < a.blocks; b += gridDim.x, first = false) {
        if (wanted) {
            // ---- phase A: c = sum_j(g^ x^q) / width of the block's rows ----
            float s = 0.0f;
            for (size_t round = 0; round < rounds; ++round) {
                const size_t tl = round * kGroups + grp, j0 = tl * kTileCols;
                const bool have = tl < across;
                const size_t cols = !have ? 0 : width - j0 < static_cast<size_t>(kTileCols) ? width - j0 : kTileCols;
                const int par = static_cast<int>(round & 1);
                load_cells<FMT>(image[par][grp], codes, b, j0, width, cols, u);
                if (static_cast<size_t>(u) < cols) scale_s[par][grp][u] = a.cells[b * width + j0 + u];
                __syncthreads();                       // (round i + 1 writes the other image, last read in round i - 1: in front of this barrier)
                if (have) {
                    float xq[kBlock], up[kBlock], ghat[kBlock];
                    piece(par, b, j0, cols, xq, up, ghat);
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) s = add_rn(s, mul_rn(ghat[k], xq[k]));
                }
            }
            s = eight_sum(s);
            if ((u & 7) == 0) part_s[grp][lrow] = s;
            __syncthreads();
            if (t < kRows) c_s[t] = div_rn(add_rn(add_rn(add_rn(part_s[0][t], part_s[1][t]), part_s[2][t]), part_s[3][t]), count);
            __syncthreads();
        }
        // ---- phase B: dres and dbranch, and the column sums of gy * x^q down the block ----
        const size_t r = kRows * b + lrow;
        const float rstd = wanted && r < rows ? a.rstd[r] : 0.0f, cr = wanted ? c_s[lrow] : 0.0f;
        for (size_t round = 0; round < rounds; ++round) {
            const size_t tl = round * kGroups + grp, j0 = tl * kTileCols;
            const bool have = tl < across;
            const size_t cols = !have ? 0 : width - j0 < static_cast<size_t>(kTileCols) ? width - j0 : kTileCols;
            load_cells<FMT>(image[0][grp], codes, b, j0, width, cols, u);
            if (static_cast<size_t>(u) < cols) scale_s[0][grp][u] = a.cells[b * width + j0 + u];
            __syncthreads();
            if (have) {
                float xq[kBlock], up[kBlock], ghat[kBlock];
                piece(0, b, j0, cols, xq, up, ghat);
                if (wanted) {
                    const size_t col = j0 + lcol;
                    T rd[kBlock];
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) rd[k] = narrow<DT>(mul_rn(rstd, sub_rn(ghat[k], mul_rn(xq[k], cr))));      // dx, as the plain kernel rounds it
                    if (gh != nullptr) {
                        T ra[kBlock];
                        load_piece<DT>(gh, a.ld_gh, a.vec_gh, r, col, rows, width, ra);
#pragma unroll
                        for (int k = 0; k < kBlock; ++k) rd[k] = narrow<DT>(add_rn(float_of_bits(widen<DT>(rd[k])), float_of_bits(widen<DT>(ra[k]))));
                    }
                    if (dres != nullptr) store_piece<DT>(dres, a.ld_dres, a.vec_dres, r, col, rows, width, rd);
                    if (dbranch != nullptr) {
                        uint32_t w[4];
                        piece_mask(r, col, width, mask_key, a.threshold, w);
#pragma unroll
                        for (int k = 0; k < kBlock; ++k) rd[k] = dropped_gradient<DT>(rd[k], mask_bits(w, k) >= a.threshold, a.scale);
                        store_piece<DT>(dbranch, a.ld_dbranch, a.vec_dbranch, r, col, rows, width, rd);
                    }
                }
                if (mine != nullptr) {
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) tile[grp][lrow][lcol + k] = mul_rn(up[k], xq[k]);
                }
            }
            __syncthreads();
            if (mine != nullptr && u < kTileCols && static_cast<size_t>(u) < cols) {
                float sum = tile[grp][0][u];
#pragma unroll 8
                for (int k = 1; k < kRows; ++k) sum = add_rn(sum, tile[grp][k][u]);
                mine[j0 + u] = first ? sum : add_rn(mine[j0 + u], sum);
            }
            // (no barrier here: backward_kernel)
        }
    }
}


}  // namespace mxnorm
}  // namespace quant
}  // namespace fewbit_hip

using namespace fewbit_hip::quant;
using fewbit_hip::sketch::key_of;

extern "C" {

size_t fewbit_hipx_mx_rms_norm_workspace(size_t rows, size_t width) { return mxnorm::workspace_of(rows, width); }

int fewbit_hipx_mx_rms_norm_forward(int dtype, const void *x, size_t ld_x, size_t rows, size_t width, const void *gamma, float eps, int format, uint64_t seed,
                                    const uint64_t *seed_device, void *y, size_t ld_y, float *rstd, uint8_t *cells, size_t cells_bytes, void *stream) {
    using namespace mxnorm;
    const char *name = "mx_rms_norm_forward";
    if (const int rc = check_call(name, dtype, format, seed_device, rows, width)) return rc;
    if (x == nullptr || gamma == nullptr || y == nullptr || rstd == nullptr || cells == nullptr) return refuse_null(name);
    if (ld_x < width || ld_y < width)
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: a row stride ld (%zu, %zu) must be at least width = %zu", name, ld_x, ld_y, width);
    const size_t item = size_of(dtype);
    if (misaligned(x, item) || misaligned(y, item) || misaligned(gamma, item) || misaligned(rstd, sizeof(float)))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: x, y, gamma and rstd must be aligned to their element size", name);
    if (const int rc = check_aligned16(name, "cells", cells)) return rc;
    if (const int rc = check_bytes(name, "cells", cells_bytes, fewbit_hip::mx::bytes_of(rows, width, format))) return rc;
    const size_t blocks = fewbit_hip::mx::blocks_of(rows);
    const ForwardArgs a{x, ld_x, rows, width, gamma, eps, key_of(seed), reinterpret_cast<const Key *>(seed_device), y, ld_y, rstd, cells, blocks,
                        wide(x, ld_x, dtype), wide(y, ld_y, dtype), wide(gamma, 0, dtype)};
    const unsigned grid = static_cast<unsigned>(blocks < kMaxGridForward ? blocks : kMaxGridForward);
    pick_kernel(dtype, format, [&](auto dt, auto fmt) {
        hipLaunchKernelGGL((forward_kernel<dt(), fmt()>), dim3(grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

int fewbit_hipx_mx_rms_norm_backward(int dtype, const void *gy, size_t ld_gy, const uint8_t *cells, size_t cells_bytes, const float *rstd, const void *gamma,
                                     size_t rows, size_t width, int format, void *dx, size_t ld_dx, float *dgamma, void *workspace, size_t workspace_bytes,
                                     void *stream) {
    using namespace mxnorm;
    const char *name = "mx_rms_norm_backward";
    if (const int rc = check_call(name, dtype, format, nullptr, rows, width)) return rc;
    if (gy == nullptr || cells == nullptr || rstd == nullptr || gamma == nullptr || (dgamma != nullptr && workspace == nullptr)) return refuse_null(name);
    if (ld_gy < width || (dx != nullptr && ld_dx < width))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: a row stride ld (%zu, %zu) must be at least width = %zu", name, ld_gy, ld_dx, width);
    const size_t item = size_of(dtype);
    if (misaligned(gy, item) || misaligned(dx, item) || misaligned(gamma, item) || misaligned(rstd, sizeof(float)) || misaligned(dgamma, sizeof(float)) ||
        misaligned(workspace, sizeof(float)))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: gy, dx, gamma, rstd, dgamma and the workspace must be aligned to their element size", name);
    if (const int rc = check_aligned16(name, "cells", cells)) return rc;
    if (const int rc = check_bytes(name, "cells", cells_bytes, fewbit_hip::mx::bytes_of(rows, width, format))) return rc;
    if (dgamma != nullptr)
        if (const int rc = check_bytes(name, "the workspace", workspace_bytes, workspace_of(rows, width))) return rc;
    if (dx == nullptr && dgamma == nullptr) return FEWBIT_OK;
    const size_t grid = backward_grid(rows);
    const BackwardArgs a{gy, ld_gy, cells, rstd, gamma, rows, width, dx, ld_dx, dgamma != nullptr ? static_cast<float *>(workspace) : nullptr,
                         fewbit_hip::mx::blocks_of(rows), wide(gy, ld_gy, dtype), wide(dx, ld_dx, dtype), wide(gamma, 0, dtype)};
    pick_kernel(dtype, format, [&](auto dt, auto fmt) {
        hipLaunchKernelGGL((backward_kernel<dt(), fmt()>), dim3(static_cast<unsigned>(grid)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    });
    if (dgamma != nullptr)
        hipLaunchKernelGGL(column_sums_kernel, dim3(static_cast<unsigned>((width + kTileCols - 1) / kTileCols)), dim3(kThreads), 0,
                           static_cast<hipStream_t>(stream), static_cast<const float *>(workspace), grid, width, dgamma);
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

int fewbit_hipx_mx_add_rms_norm_forward(int dtype, const void *x, size_t ld_x, const void *residual, size_t ld_residual, size_t rows, size_t width,
                                        const void *gamma, float eps, int format, uint64_t seed, uint64_t seed_mask, const uint64_t *seed_device,
                                        uint32_t threshold, void *y, size_t ld_y, void *h_out, size_t ld_h, float *rstd, uint8_t *cells, size_t cells_bytes,
                                        void *stream) {
    using namespace mxnorm;
    const char *name = "mx_add_rms_norm_forward";
    if (const int rc = check_call(name, dtype, format, seed_device, rows, width)) return rc;
    if (const int rc = check_mask(name, threshold, width)) return rc;
    if (residual == nullptr) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: null pointer (residual)", name);
    if (x == nullptr || gamma == nullptr || y == nullptr || rstd == nullptr || cells == nullptr) return refuse_null(name);
    if (ld_x < width || ld_residual < width || ld_y < width || (h_out != nullptr && ld_h < width))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: a row stride ld (%zu, %zu, %zu, %zu) must be at least width = %zu", name, ld_x, ld_residual, ld_y, ld_h, width);
    const size_t item = size_of(dtype);
    if (misaligned(x, item) || misaligned(residual, item) || misaligned(y, item) || misaligned(h_out, item) || misaligned(gamma, item) ||
        misaligned(rstd, sizeof(float)))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: x, residual, y, h_out, gamma and rstd must be aligned to their element size", name);
    if (const int rc = check_aligned16(name, "cells", cells)) return rc;
    if (const int rc = check_bytes(name, "cells", cells_bytes, fewbit_hip::mx::bytes_of(rows, width, format))) return rc;
    const size_t blocks = fewbit_hip::mx::blocks_of(rows);
    const AddForwardArgs a{x, residual, ld_x, ld_residual, rows, width, gamma, eps, key_of(seed), key_of(seed_mask), reinterpret_cast<const Key *>(seed_device),
                           threshold, fewbit_hip::unit::scale_of(threshold), y, h_out, ld_y, ld_h, rstd, cells, blocks,
                           wide(x, ld_x, dtype), wide(residual, ld_residual, dtype), wide(y, ld_y, dtype), wide(h_out, ld_h, dtype), wide(gamma, 0, dtype)};
    const unsigned grid = static_cast<unsigned>(blocks < kMaxGridForward ? blocks : kMaxGridForward);
    pick_kernel(dtype, format, [&](auto dt, auto fmt) {
        hipLaunchKernelGGL((add_forward_kernel<dt(), fmt()>), dim3(grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

int fewbit_hipx_mx_add_rms_norm_backward(int dtype, const void *gy, size_t ld_gy, const void *gh, size_t ld_gh, const uint8_t *cells, size_t cells_bytes,
                                         const float *rstd, const void *gamma, size_t rows, size_t width, int format, uint64_t seed_mask,
                                         const uint64_t *seed_device, uint32_t threshold, void *dres, size_t ld_dres, void *dbranch, size_t ld_dbranch,
                                         float *dgamma, void *workspace, size_t workspace_bytes, void *stream) {
    using namespace mxnorm;
    const char *name = "mx_add_rms_norm_backward";
    if (const int rc = check_call(name, dtype, format, seed_device, rows, width)) return rc;
    if (const int rc = check_mask(name, threshold, width)) return rc;
    if (dbranch != nullptr && threshold == 0)
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: with threshold = 0 dbranch is dres: pass dbranch = NULL", name);
    if (gy == nullptr || cells == nullptr || rstd == nullptr || gamma == nullptr || (dgamma != nullptr && workspace == nullptr)) return refuse_null(name);
    if (ld_gy < width || (gh != nullptr && ld_gh < width) || (dres != nullptr && ld_dres < width) || (dbranch != nullptr && ld_dbranch < width))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: a row stride ld (%zu, %zu, %zu, %zu) must be at least width = %zu", name, ld_gy, ld_gh, ld_dres, ld_dbranch,
                    width);
    const size_t item = size_of(dtype);
    if (misaligned(gy, item) || misaligned(gh, item) || misaligned(dres, item) || misaligned(dbranch, item) || misaligned(gamma, item) ||
        misaligned(rstd, sizeof(float)) || misaligned(dgamma, sizeof(float)) || misaligned(workspace, sizeof(float)))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: gy, gh, dres, dbranch, gamma, rstd, dgamma and the workspace must be aligned to their element size", name);
    if (const int rc = check_aligned16(name, "cells", cells)) return rc;
    if (const int rc = check_bytes(name, "cells", cells_bytes, fewbit_hip::mx::bytes_of(rows, width, format))) return rc;
    if (dgamma != nullptr)
        if (const int rc = check_bytes(name, "the workspace", workspace_bytes, workspace_of(rows, width))) return rc;
    if (dres == nullptr && dbranch == nullptr && dgamma == nullptr) return FEWBIT_OK;
    const size_t grid = backward_grid(rows);
    const AddBackwardArgs a{gy, gh, ld_gy, ld_gh, cells, rstd, gamma, rows, width, key_of(seed_mask), reinterpret_cast<const Key *>(seed_device), threshold,
                            fewbit_hip::unit::scale_of(threshold), dres, dbranch, ld_dres, ld_dbranch, dgamma != nullptr ? static_cast<float *>(workspace) : nullptr,
                            fewbit_hip::mx::blocks_of(rows), wide(gy, ld_gy, dtype), wide(gh, ld_gh, dtype), wide(dres, ld_dres, dtype),
                            wide(dbranch, ld_dbranch, dtype), wide(gamma, 0, dtype)};
    pick_kernel(dtype, format, [&](auto dt, auto fmt) {
        hipLaunchKernelGGL((add_backward_kernel<dt(), fmt()>), dim3(static_cast<unsigned>(grid)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    });
    if (dgamma != nullptr)
        hipLaunchKernelGGL(column_sums_kernel, dim3(static_cast<unsigned>((width + kTileCols - 1) / kTileCols)), dim3(kThreads), 0,
                           static_cast<hipStream_t>(stream), static_cast<const float *>(workspace), grid, width, dgamma);
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

}  // extern "C"
