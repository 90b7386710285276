// fewbit_mxlnorm.hip -- the LAYER norm in front of linear layers that keep their input as OCP-MX cells: the norm keeps its normalized rows
// x^ = (x - mean) * rstd as ONE mx_pack buffer and one fp32 rstd per row, which serve its own backward and, because y = x^ * gamma + beta, every weight
// gradient behind it (dW = (G^T x^) * gamma by columns + (sum_rows G) (x) beta: mx_wgrad on the cells as they lie, and the bias gradient the linear
// has anyway), on gfx950; part of the companion library libfewbit_hipx.so (include/fewbit_hipx.h, "The centred normalized rows as row blocks"):
//
//     mx_layer_norm_forward    x, gamma, beta -> y, mean, rstd and the cells of the FP32 x^                                            ONE launch
//     mx_layer_norm_backward   gy, the cells, rstd, gamma -> dx, and the workgroups' column sums of gy * x^q and of gy -> dgamma, dbeta
//                                                                                                              ONE launch and a small one
//
// The format is fewbit_mxdef.h's, the formulas are those of fewbit_norm.hip's centred kind, the geometry and the two roles of a tile are
// fewbit_mxrows.h's (shared with the RMS unit fewbit_mxnorm.hip, whose kernels cannot serve here: a centred two-pass statistic, beta in the forward,
// two row sums and two sets of column sums in the backward).  What this unit chose:
//   workgroup  1024 lanes own ONE row block b (32 rows) and walk on by the grid's width: a row's statistics are known before the row is rounded,
//              with no flag or atomic between workgroups.  Planned and reported by the compiler: no scratch, at most 128 registers a lane, so ONE
//              workgroup (16 waves) on a compute unit, which leaves it all of the 160 KiB of LDS; the backward takes about 80 KiB.
//   forward A  wave w takes rows w and w + 16 of the block and makes TWO passes over the row's 8-element pieces (piece l, l + 64, .. of lane l):
//              the sum of x, each lane in index order, then the DPP / readlane order of mxrows::wave_sum; mean = sum / width; then the sum of
//              (x - mean)^2 over the same pieces in the same order (the row is read again: the same wave has just fetched it, it comes from L2 or
//              nearer; a missing element counts +0 in both sums).  rstd = 1 / sqrt(sum / width + eps).  mean and rstd -> LDS and the outputs.
//              ONE plan at every width, nothing held in registers between the passes: cabi_x.MX_NORM_PLAN_WIDTHS stays empty.
//   forward B  the block's 32 x 64 tiles, FOUR in flight, each on its own group of 256 lanes, with the two roles of mx::pack_kernel:
//              load role   lane u: row u / 8, columns 8 (u % 8) .. + 7: x again, x^ = (x - mean) * rstd, y = round(x^ * gamma + beta) stored, the
//                          fp32 x^ into the group's LDS tile.
//              round role  lane u: column u % 64, row octet u / 64: the text of the RMS unit.  3 barriers a round of four tiles.
//   backward A (only where dx is wanted) ONE sweep over the cells gives BOTH row sums, of g^ and of g^ x^q.  Cell images come into LDS by 8-byte
//              pieces, alternating between two images so that ONE barrier a round suffices.  The image is laid out in dwords with one dword of
//              padding behind every eight cells, and a lane reads the dword (fp4) or the two dwords (fp6) that hold its row octet of a cell: the
//              eight lanes of a tile row, whose cells are 8 apart, fall into eight different banks (33 q and 49 q modulo 32 and modulo 64 are
//              distinct for q = 0 .. 7), and the eight rows of a wave share an octet, so they read the same dword (a broadcast).  The eight scale
//              bytes of a lane are one 8-byte read.  A lane adds its terms in index order; the partial sums of a row meet in a fixed order: the
//              eight lanes by DPP (^1, ^2, the other quad), then the four groups in ascending order through LDS.  c1, c2 = sum / width.
//   backward B the tiles again: dx = round(rstd * ((g^ - c1) - x^q c2)) stored; gy * x^q and gy -> the group's two LDS tiles.  ALL FOUR waves of a
//              group add columns: wave v takes quantity v % 2 (0: gy * x^q, 1: gy) and the 32 columns from 32 (v / 2); lanes 0 .. 31 add rows
//              0 .. 15 of their column in ascending order, lanes 32 .. 63 rows 16 .. 31 (their half of the tile lies 32 floats further on, so that
//              the two halves read different banks), the halves meet as (rows 0 .. 15) + (rows 16 .. 31) through one ds_bpermute, and the lower
//              half adds the result into the workgroup's row of the workspace [workgroups][2][width] (the same lane owns a column at every row
//              block the workgroup walks: a plain read-add-write of its own).  2 barriers a round.
//   column sums  a second launch, a workgroup per 64 columns of each quantity, adds the workgroups' rows in ascending order, associated by
//              sixteenths (mxrows::add_partials) -> dgamma and dbeta.  At most kMaxGridBackward workgroups wrote rows.
// Every sum is in an order fixed by the shape alone; there are no atomics: the same arguments give the same bytes.
// NOT done (EXPERIMENTS.md 8.35): phase B decodes the cells a second time from LDS instead of carrying phase A's code dwords in registers (a row
// block of 8192 columns is 32 tiles a lane), and phase B keeps its two barriers a round.
// Rows beyond `rows` count as +0 (their mean and rstd are taken as 0), columns beyond `width` are neither rounded into a stored cell nor stored.
// Roofline class: memory (forward reads x once from memory and twice from L2, writes y and 0.27 / 0.39 of it in cells).
//
// The sum of a seed in front of it (include/fewbit_hipx.h, "The sum of a seed in front of the centred normalized rows"): h = residual + dropout(x)
// normalized in the same launch, and the gradients of both behind the norm's backward:
//
//     mx_add_layer_norm_forward    x, residual, gamma, beta -> y, mean, rstd, the cells of h^ and, where asked for, h                      ONE launch
//     mx_add_layer_norm_backward   gy, [gy_add], [gh], the cells, rstd, gamma -> dres, dbranch, the column sums -> dgamma, dbeta
//                                                                                                              ONE launch and a small one
//
// Two kernels of their own (add_forward_kernel, add_backward_kernel) beside the plain pair, whose text and code stay as they were; the walk, the
// roles, the barriers and every sum's order are the plain kernels', so that every output is bit for bit fewbit_hipx_dropout with the residual as
// addend, the plain entry point, and torch's addition of two tensors.  What the fusion had to settle:
//   h thrice   the centred statistic takes two passes over a row and the tiles a third; each forms h = narrow(x scale + residual) from x, the
//              residual and the mask (mxrows::sum_piece: two 16-byte loads and one Philox call per eight elements), and because h is ROUNDED to the
//              dtype before anything reads it the three agree bit for bit.  x and the residual come from memory once and from L2 twice.  Nothing of
//              a row is held between the passes and h is never read back: ONE plan at every width, with or without h_out, which the tile pass
//              stores (its lanes hold the piece they store anyway; phase A's waves would write the same lines a second way).
//   the mask   is drawn on blocks of eight FLAT elements; with width % 8 == 0 a lane's piece in the load role is one flat block in all three
//              walks.  threshold = 0 draws nothing and serves every width; a mask at another width is refused.
//   gy_add     the gradient that arrives at the norm's own output (y feeds the next residual, post-norm) is added where a piece of gy is
//              loaded, in BOTH phases, rounded to the dtype as torch's gy.add_ rounds it: the row sums, dx and both column sums see the same g.
//   backward   phase B rounds dx as the plain kernel does, adds gh as torch adds two tensors -> dres, and draws the piece's mask for
//              dbranch = keep ? narrow(dres scale) : +0.  With threshold = 0 dbranch is dres and must be absent.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fewbit_hipx.h"
#include "fewbit_mxdef.h"
#include "fewbit_mxrows.h"

#pragma clang fp contract(off)

namespace fewbit_hip {
namespace quant {
namespace mxlnorm {

using namespace mxrows;

constexpr int kSums = 2;                    // the quantities of the backward: gy * x^q (dgamma), gy (dbeta)
constexpr int kHalfRows = kRows / 2, kHalfShift = 32, kTileFloats = kRows * kTileCols + kHalfShift;

inline size_t workspace_of(size_t rows, size_t width) { return known_shape(rows, width) ? backward_grid(rows) * kSums * width * sizeof(float) : 0; }

struct ForwardArgs {
    const void *x;
    size_t ld_x, rows, width;
    const void *gamma, *beta;               // beta may be absent: it counts as 0 and nothing is added
    float eps;
    Key key;
    const Key *device;                      // nullptr, or the key in device memory
    void *y;
    size_t ld_y;
    float *mean, *rstd;
    uint8_t *cells;
    size_t blocks;
    bool vec_x, vec_y, vec_gamma, vec_beta;
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
    __shared__ float mean_s[kRows], rstd_s[kRows];
    __shared__ uint32_t tile[kGroups][kRows][kTileCols];                        // the fp32 bits of x^
    __shared__ uint32_t amax_s[kGroups][kOctets][kTileCols];
    __shared__ uint64_t image[kGroups][kTileCols * kCell / 8];
    const T *x = static_cast<const T *>(a.x), *gamma = static_cast<const T *>(a.gamma), *beta = static_cast<const T *>(a.beta);
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
        // ---- phase A: the two statistics of the block's rows, a wave per row, two passes over the same pieces in the same order ----
        for (int lr = wave; lr < kRows; lr += kWaves) {
            const size_t r = kRows * b + lr;
            float s = 0.0f;
            if (r < rows) {
                for (size_t p = lane; p < pieces; p += 64) {
                    T raw[kBlock];
                    load_piece<DT>(x, a.ld_x, a.vec_x, r, kBlock * p, rows, width, raw);
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) s = add_rn(s, float_of_bits(widen<DT>(raw[k])));      // (a missing element: +0)
                }
            }
            const float mean = div_rn(wave_sum(s), count);
            float ss = 0.0f;
            if (r < rows) {
                for (size_t p = lane; p < pieces; p += 64) {
                    T raw[kBlock];
                    load_piece<DT>(x, a.ld_x, a.vec_x, r, kBlock * p, rows, width, raw);
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) {
                        const float d = kBlock * p + k < width ? sub_rn(float_of_bits(widen<DT>(raw[k])), mean) : 0.0f;
                        ss = add_rn(ss, mul_rn(d, d));
                    }
                }
            }
            const float rstd = div_rn(1.0f, sqrt_rn(add_rn(div_rn(wave_sum(ss), count), a.eps)));
            if (lane == 0) {
                mean_s[lr] = r < rows ? mean : 0.0f;
                rstd_s[lr] = r < rows ? rstd : 0.0f;
                if (r < rows) a.mean[r] = mean, a.rstd[r] = rstd;
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
                T rx[kBlock], rg[kBlock], rb[kBlock], ry[kBlock];
                load_piece<DT>(x, a.ld_x, a.vec_x, r, col, rows, width, rx);
                load_piece<DT>(gamma, 0, a.vec_gamma, 0, col, 1, width, rg);
                if (beta != nullptr) load_piece<DT>(beta, 0, a.vec_beta, 0, col, 1, width, rb);
                const float mean = mean_s[lrow], rstd = rstd_s[lrow];
#pragma unroll
                for (int k = 0; k < kBlock; ++k) {
                    const float xhat = mul_rn(sub_rn(float_of_bits(widen<DT>(rx[k])), mean), rstd);
                    const float scaled = mul_rn(xhat, float_of_bits(widen<DT>(rg[k])));
                    ry[k] = narrow<DT>(beta != nullptr ? add_rn(scaled, float_of_bits(widen<DT>(rb[k]))) : scaled);
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
            // writes mean_s and rstd_s behind the reads in front of this round's first: no barrier here)
        }
    }
}

// ---- the padded dword image of a tile's cells: cell c begins at dword FMT c + c / 8 (a cell is FMT dwords) -----------------------------------------
template <int FMT> constexpr int image_words() { return kTileCols * FMT + kTileCols / 8; }
template <int FMT> __device__ __forceinline__ void load_image(uint32_t *image, const uint8_t *codes, size_t b, size_t j0, size_t width, size_t cols, int u) {
    if (2 * static_cast<size_t>(u) < cols * FMT) {                              // 8-byte pieces, consecutive lanes consecutive pieces
        const uint64_t piece = reinterpret_cast<const uint64_t *>(codes + (b * width + j0) * mx::cell_bytes(FMT))[u];
        const int d = 2 * u, at = d + d / (8 * FMT);                            // (8 FMT is even: both dwords of a piece lie in front of the same padding)
        image[at] = static_cast<uint32_t>(piece), image[at + 1] = static_cast<uint32_t>(piece >> 32);
    }
}
// element `row` of the cell of tile column `c`: the dword(s) of the row's octet, then the code
template <int FMT> __device__ __forceinline__ uint32_t image_code(const uint32_t *image, int c, int row) {
    const int base = FMT * c + (c >> 3), o = row >> 3, e = row & 7;
    if constexpr (FMT == 4) {
        return (image[base + o] >> (4 * e)) & 0xFu;
    } else {
        const int d0 = (3 * o) >> 1;                                            // the octet's 48 bits begin at bit 48 o of the cell
        const uint64_t two = static_cast<uint64_t>(image[base + d0]) | static_cast<uint64_t>(image[base + d0 + 1]) << 32;
        return static_cast<uint32_t>(two >> (16 * (o & 1) + 6 * e)) & 0x3Fu;
    }
}
__device__ __forceinline__ int tile_at(int row, int col) { return row * kTileCols + col + (row >= kHalfRows ? kHalfShift : 0); }

template <int DT, int FMT>
__global__ __launch_bounds__(kThreads) void backward_kernel(BackwardArgs a) {
    using T = typename Elem<DT>::type;
    __shared__ uint32_t image[2][kGroups][image_words<FMT>()];
    __shared__ uint64_t scale_s[2][kGroups][kTileCols / 8];
    __shared__ float tile[kGroups][kSums][kTileFloats];                         // gy * x^q, gy
    __shared__ float part_s[kSums][kGroups][kRows], c_s[kSums][kRows];
    const T *gy = static_cast<const T *>(a.gy), *gamma = static_cast<const T *>(a.gamma);
    T *dx = static_cast<T *>(a.dx);
    const size_t rows = a.rows, width = a.width;
    const uint8_t *codes = a.cells + mx::codes_offset(rows, width);
    float *mine = a.partials != nullptr ? a.partials + static_cast<size_t>(blockIdx.x) * kSums * width : nullptr;
    const int t = threadIdx.x;
    const int grp = t >> 8, u = t & (kGroupThreads - 1);
    const int lrow = u >> 3, lcol = 8 * (u & 7);          // the load role
    const int which = (u >> 6) & 1, half = (u >> 5) & 1, ccol = 32 * (u >> 7) + (u & 31);       // the adding role: quantity, half of the rows, column
    const size_t across = (width + kTileCols - 1) / kTileCols, rounds = (across + kGroups - 1) / kGroups;
    const float count = static_cast<float>(width);
    auto fetch = [&](int par, size_t b, size_t j0, size_t cols) {
        load_image<FMT>(image[par][grp], codes, b, j0, width, cols, u);
        if (static_cast<size_t>(u) < cols) reinterpret_cast<uint8_t *>(scale_s[par][grp])[u] = a.cells[b * width + j0 + u];
    };
    // the eight x^q, gy and g^ of the lane's piece of tile (b, j0) from the LDS image `par`
    auto piece = [&](int par, size_t b, size_t j0, size_t cols, float (&xq)[kBlock], float (&up)[kBlock], float (&gh)[kBlock]) {
        const size_t r = kRows * b + lrow, col = j0 + lcol;
        T rgy[kBlock], rg[kBlock];
        load_piece<DT>(gy, a.ld_gy, a.vec_gy, r, col, rows, width, rgy);
        load_piece<DT>(gamma, 0, a.vec_gamma, 0, col, 1, width, rg);
        const uint64_t scales = scale_s[par][grp][u & 7];
#pragma unroll
        for (int k = 0; k < kBlock; ++k) {
            const bool inside = r < rows && lcol + k < static_cast<int>(cols);
            xq[k] = inside ? mx::decode<FMT>(image_code<FMT>(image[par][grp], lcol + k, lrow), static_cast<uint32_t>(scales >> (8 * k)) & 0xFFu) : 0.0f;
            up[k] = float_of_bits(widen<DT>(rgy[k]));                           // (outside: +0)
            gh[k] = mul_rn(up[k], float_of_bits(widen<DT>(rg[k])));
        }
    };
    bool first = true;                                                          // of this workgroup's row blocks: its rows of the workspace are written, not added to
    for (size_t b = blockIdx.x; b < a.blocks; b += gridDim.x, first = false) {
        if (dx != nullptr) {
            // ---- phase A: c1 = sum_j(g^) / width and c2 = sum_j(g^ x^q) / width of the block's rows, ONE sweep ----
            float s1 = 0.0f, s2 = 0.0f;
            for (size_t round = 0; round < rounds; ++round) {
                const size_t tl = round * kGroups + grp, j0 = tl * kTileCols;
                const bool have = tl < across;
                const size_t cols = !have ? 0 : width - j0 < static_cast<size_t>(kTileCols) ? width - j0 : kTileCols;
                const int par = static_cast<int>(round & 1);
                fetch(par, b, j0, cols);
                __syncthreads();                       // (round i + 1 writes the other image, last read in round i - 1: in front of this barrier)
                if (have) {
                    float xq[kBlock], up[kBlock], gh[kBlock];
                    piece(par, b, j0, cols, xq, up, gh);
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) {
                        s1 = add_rn(s1, gh[k]);
                        s2 = add_rn(s2, mul_rn(gh[k], xq[k]));
                    }
                }
            }
            s1 = eight_sum(s1), s2 = eight_sum(s2);
            if ((u & 7) == 0) part_s[0][grp][lrow] = s1, part_s[1][grp][lrow] = s2;
            __syncthreads();
            if (t < kSums * kRows) {
                const int q = t >> 5, row = t & (kRows - 1);
                c_s[q][row] = div_rn(add_rn(add_rn(add_rn(part_s[q][0][row], part_s[q][1][row]), part_s[q][2][row]), part_s[q][3][row]), count);
            }
            __syncthreads();
        }
        // ---- phase B: dx, and the column sums of gy * x^q and of gy down the block ----
        const size_t r = kRows * b + lrow;
        const float rstd = dx != nullptr && r < rows ? a.rstd[r] : 0.0f;
        const float c1 = dx != nullptr ? c_s[0][lrow] : 0.0f, c2 = dx != nullptr ? c_s[1][lrow] : 0.0f;
        for (size_t round = 0; round < rounds; ++round) {
            const size_t tl = round * kGroups + grp, j0 = tl * kTileCols;
            const bool have = tl < across;
            const size_t cols = !have ? 0 : width - j0 < static_cast<size_t>(kTileCols) ? width - j0 : kTileCols;
            fetch(0, b, j0, cols);
            __syncthreads();
            if (have) {
                float xq[kBlock], up[kBlock], gh[kBlock];
                piece(0, b, j0, cols, xq, up, gh);
                if (dx != nullptr) {
                    T rdx[kBlock];
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) rdx[k] = narrow<DT>(mul_rn(rstd, sub_rn(sub_rn(gh[k], c1), mul_rn(xq[k], c2))));
                    store_piece<DT>(dx, a.ld_dx, a.vec_dx, r, j0 + lcol, rows, width, rdx);
                }
                if (mine != nullptr) {
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) {
                        tile[grp][0][tile_at(lrow, lcol + k)] = mul_rn(up[k], xq[k]);
                        tile[grp][1][tile_at(lrow, lcol + k)] = up[k];
                    }
                }
            }
            __syncthreads();
            if (mine != nullptr) {                                              // (the whole workgroup alike: the exchange below takes every lane of a wave)
                const float *from = tile[grp][which];
                float sum = from[tile_at(kHalfRows * half, ccol)];
#pragma unroll 5
                for (int k = 1; k < kHalfRows; ++k) sum = add_rn(sum, from[tile_at(kHalfRows * half + k, ccol)]);
                const float other = __shfl_xor(sum, 32);                        // lanes 0 .. 31: rows 16 .. 31 of the same column
                if (half == 0 && static_cast<size_t>(ccol) < cols) {
                    const float total = add_rn(sum, other);
                    float *at = mine + which * width + j0 + ccol;
                    *at = first ? total : add_rn(*at, total);
                }
            }
            // (the next round writes the image behind this round's second barrier, and `tile` behind its own first: no barrier here)
        }
    }
}

// dgamma (blockIdx.y = 0) and dbeta (1): the workgroups' sums of 64 columns of one quantity; an absent output is not written
__global__ __launch_bounds__(kThreads) void column_sums_kernel(const float *__restrict__ partials, size_t parts, size_t width, float *__restrict__ dgamma,
                                                               float *__restrict__ dbeta) {
    __shared__ float waves[kWaves][kTileCols];
    float *dst = blockIdx.y == 0 ? dgamma : dbeta;
    if (dst == nullptr) return;
    add_partials(partials + blockIdx.y * width, parts, kSums * width, width, blockIdx.x, dst, waves);
}

// ---- the sum of a seed in front of the norm: h = residual + dropout(x), and the gradients of the two behind the norm's backward -------------------
struct AddForwardArgs {
    const void *x, *residual;
    size_t ld_x, ld_res, rows, width;
    const void *gamma, *beta;               // beta may be absent: it counts as 0 and nothing is added
    float eps;
    Key key, mask_key;
    const Key *device;                      // nullptr, or the two keys in device memory: the cells', then the mask's
    uint32_t threshold;
    float scale;
    void *y, *h;                            // h may be absent: it is then not written
    size_t ld_y, ld_h;
    float *mean, *rstd;                     // mean may be absent
    uint8_t *cells;
    size_t blocks;
    bool vec_x, vec_res, vec_y, vec_h, vec_gamma, vec_beta;
};
struct AddBackwardArgs {
    const void *gy, *gy_add, *gh;           // gy_add and gh may each be absent: nothing is added
    size_t ld_gy, ld_add, ld_gh;
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
    bool vec_in, vec_out, vec_gamma;        // 16-byte pieces serve every gradient that is read (gy, gy_add, gh) / every one that is written
};

// v, as a value the compiler knows nothing about: what is computed from it is computed where it is used
__device__ __forceinline__ int fresh(int v) {
    asm volatile("" : "+v"(v));
    return v;
}
// forward_kernel with h = residual + dropout(x) in the place of x: formed in registers by each of the three passes (mxrows::sum_piece), stored by
// the last where h is wanted
template <int DT, int FMT>
__global__ __launch_bounds__(kThreads) void add_forward_kernel(AddForwardArgs a) {
    using T = typename Elem<DT>::type;
    constexpr size_t kCell = mx::cell_bytes(FMT);
    __shared__ float mean_s[kRows], rstd_s[kRows];
    __shared__ uint32_t tile[kGroups][kRows][kTileCols];                        // the fp32 bits of h^
    __shared__ uint32_t amax_s[kGroups][kOctets][kTileCols];
    __shared__ uint64_t image[kGroups][kTileCols * kCell / 8];
    const T *gamma = static_cast<const T *>(a.gamma), *beta = static_cast<const T *>(a.beta);
    T *y = static_cast<T *>(a.y), *h_out = static_cast<T *>(a.h);
    Key key = a.key, mask_key = a.mask_key;
    if (a.device != nullptr) key = a.device[0], mask_key = a.device[1];
    const size_t rows = a.rows, width = a.width;
    uint8_t *codes = a.cells + mx::codes_offset(rows, width);
    const size_t across = (width + kTileCols - 1) / kTileCols, rounds = (across + kGroups - 1) / kGroups, pieces = (width + kBlock - 1) / kBlock;
    const float count = static_cast<float>(width);
    for (size_t b = blockIdx.x; b < a.blocks; b += gridDim.x) {
        // (each phase takes the lane's number afresh: what a phase derives from it -- indices, addresses, conditions -- is then not carried in
        // registers through the other phase, which is what keeps this kernel within its 128 registers without scratch)
        // ---- phase A: the two statistics of the block's rows of h, a wave per row, two passes that each form the row's h ----
        const int wave = fresh(threadIdx.x) >> 6, lane = threadIdx.x & 63;
        for (int lr = wave; lr < kRows; lr += kWaves) {
            const size_t r = kRows * b + lr;
            float s = 0.0f;
            if (r < rows) {
                for (size_t p = lane; p < pieces; p += 64) {
                    T rh[kBlock];
                    sum_piece<DT>(a, mask_key, r, kBlock * p, rh);
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) s = add_rn(s, float_of_bits(widen<DT>(rh[k])));       // (a missing element: +0)
                }
            }
            const float mean = div_rn(wave_sum(s), count);
            float ss = 0.0f;
            if (r < rows) {
                for (size_t p = lane; p < pieces; p += 64) {
                    T rh[kBlock];
                    sum_piece<DT>(a, mask_key, r, kBlock * p, rh);
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) {
                        const float d = kBlock * p + k < width ? sub_rn(float_of_bits(widen<DT>(rh[k])), mean) : 0.0f;
                        ss = add_rn(ss, mul_rn(d, d));
                    }
                }
            }
            const float rstd = div_rn(1.0f, sqrt_rn(add_rn(div_rn(wave_sum(ss), count), a.eps)));
            if (lane == 0) {
                mean_s[lr] = r < rows ? mean : 0.0f;
                rstd_s[lr] = r < rows ? rstd : 0.0f;
                if (r < rows) {
                    a.rstd[r] = rstd;
                    if (a.mean != nullptr) a.mean[r] = mean;
                }
            }
        }
        __syncthreads();
        // ---- phase B: the block's tiles, four in flight ----
        const int t = fresh(threadIdx.x), grp = t >> 8, u = t & (kGroupThreads - 1);
        const int lrow = u >> 3, lcol = 8 * (u & 7);          // the load role
        const int c = u & (kTileCols - 1), o = u >> 6;        // the rounding role: column c, row octet o
        for (size_t round = 0; round < rounds; ++round) {
            const size_t tl = round * kGroups + grp, j0 = tl * kTileCols;
            const bool have = tl < across;                                      // (the same for every lane of a group; the barriers are outside)
            const size_t cols = !have ? 0 : width - j0 < static_cast<size_t>(kTileCols) ? width - j0 : kTileCols;
            if (have) {
                const size_t r = kRows * b + lrow, col = j0 + lcol;
                T rh[kBlock], rg[kBlock], rb[kBlock], ry[kBlock];
                sum_piece<DT>(a, mask_key, r, col, rh);
                if (h_out != nullptr) store_piece<DT>(h_out, a.ld_h, a.vec_h, r, col, rows, width, rh);
                load_piece<DT>(gamma, 0, a.vec_gamma, 0, col, 1, width, rg);
                if (beta != nullptr) load_piece<DT>(beta, 0, a.vec_beta, 0, col, 1, width, rb);
                const float mean = mean_s[lrow], rstd = rstd_s[lrow];
#pragma unroll
                for (int k = 0; k < kBlock; ++k) {
                    const float xhat = mul_rn(sub_rn(float_of_bits(widen<DT>(rh[k])), mean), rstd);
                    const float scaled = mul_rn(xhat, float_of_bits(widen<DT>(rg[k])));
                    ry[k] = narrow<DT>(beta != nullptr ? add_rn(scaled, float_of_bits(widen<DT>(rb[k]))) : scaled);
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

// backward_kernel with g = gy + gy_add in the place of gy, and dres = dx + gh and dbranch = the dropout's gradient of dres in the place of dx
template <int DT, int FMT>
__global__ __launch_bounds__(kThreads) void add_backward_kernel(AddBackwardArgs a) {
    using T = typename Elem<DT>::type;
    __shared__ uint32_t image[2][kGroups][image_words<FMT>()];
    __shared__ uint64_t scale_s[2][kGroups][kTileCols / 8];
    __shared__ float tile[kGroups][kSums][kTileFloats];                         // g * x^q, g
    __shared__ float part_s[kSums][kGroups][kRows], c_s[kSums][kRows];
    const T *gy = static_cast<const T *>(a.gy), *gy_add = static_cast<const T *>(a.gy_add), *gh = static_cast<const T *>(a.gh);
    const T *gamma = static_cast<const T *>(a.gamma);
    T *dres = static_cast<T *>(a.dres), *dbranch = static_cast<T *>(a.dbranch);
    Key mask_key = a.mask_key;
    if (a.device != nullptr) mask_key = *a.device;
    const bool wanted = dres != nullptr || dbranch != nullptr;
    const size_t rows = a.rows, width = a.width;
    const uint8_t *codes = a.cells + mx::codes_offset(rows, width);
    float *mine = a.partials != nullptr ? a.partials + static_cast<size_t>(blockIdx.x) * kSums * width : nullptr;
    int t, grp, u, lrow, lcol;                            // the load role, taken afresh by each phase (add_forward_kernel)
    auto take = [&] { t = fresh(threadIdx.x), grp = t >> 8, u = t & (kGroupThreads - 1), lrow = u >> 3, lcol = 8 * (u & 7); };
    const size_t across = (width + kTileCols - 1) / kTileCols, rounds = (across + kGroups - 1) / kGroups;
    const float count = static_cast<float>(width);
    auto fetch = [&](int par, size_t b, size_t j0, size_t cols) {
        load_image<FMT>(image[par][grp], codes, b, j0, width, cols, u);
        if (static_cast<size_t>(u) < cols) reinterpret_cast<uint8_t *>(scale_s[par][grp])[u] = a.cells[b * width + j0 + u];
    };
    // the eight x^q, g = gy + gy_add as rounded to the dtype, and g^ of the lane's piece of tile (b, j0) from the LDS image `par`
    auto piece = [&](int par, size_t b, size_t j0, size_t cols, float (&xq)[kBlock], float (&up)[kBlock], float (&ghat)[kBlock]) {
        const size_t r = kRows * b + lrow, col = j0 + lcol;
        T rgy[kBlock], rg[kBlock];
        load_piece<DT>(gy, a.ld_gy, a.vec_in, r, col, rows, width, rgy);
        if (gy_add != nullptr) {
            T ra[kBlock];
            load_piece<DT>(gy_add, a.ld_add, a.vec_in, r, col, rows, width, ra);
#pragma unroll
            for (int k = 0; k < kBlock; ++k) rgy[k] = added<DT>(rgy[k], ra[k]);
        }
        load_piece<DT>(gamma, 0, a.vec_gamma, 0, col, 1, width, rg);
        const uint64_t scales = scale_s[par][grp][u & 7];
#pragma unroll
        for (int k = 0; k < kBlock; ++k) {
            const bool inside = r < rows && lcol + k < static_cast<int>(cols);
            xq[k] = inside ? mx::decode<FMT>(image_code<FMT>(image[par][grp], lcol + k, lrow), static_cast<uint32_t>(scales >> (8 * k)) & 0xFFu) : 0.0f;
            up[k] = float_of_bits(widen<DT>(rgy[k]));                           // (outside: +0)
            ghat[k] = mul_rn(up[k], float_of_bits(widen<DT>(rg[k])));
        }
    };
    bool first = true;                                                          // of this workgroup's row blocks: its rows of the workspace are written, not added to
    for (size_t b = blockIdx.x; b < a.blocks; b += gridDim.x, first = false) {
        if (wanted) {
            // ---- phase A: c1 = sum_j(g^) / width and c2 = sum_j(g^ x^q) / width of the block's rows, ONE sweep ----
            take();
            float s1 = 0.0f, s2 = 0.0f;
            for (size_t round = 0; round < rounds; ++round) {
                const size_t tl = round * kGroups + grp, j0 = tl * kTileCols;
                const bool have = tl < across;
                const size_t cols = !have ? 0 : width - j0 < static_cast<size_t>(kTileCols) ? width - j0 : kTileCols;
                const int par = static_cast<int>(round & 1);
                fetch(par, b, j0, cols);
                __syncthreads();                       // (round i + 1 writes the other image, last read in round i - 1: in front of this barrier)
                if (have) {
                    float xq[kBlock], up[kBlock], ghat[kBlock];
                    piece(par, b, j0, cols, xq, up, ghat);
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) {
                        s1 = add_rn(s1, ghat[k]);
                        s2 = add_rn(s2, mul_rn(ghat[k], xq[k]));
                    }
                }
            }
            s1 = eight_sum(s1), s2 = eight_sum(s2);
            if ((u & 7) == 0) part_s[0][grp][lrow] = s1, part_s[1][grp][lrow] = s2;
            __syncthreads();
            if (t < kSums * kRows) {
                const int q = t >> 5, row = t & (kRows - 1);
                c_s[q][row] = div_rn(add_rn(add_rn(add_rn(part_s[q][0][row], part_s[q][1][row]), part_s[q][2][row]), part_s[q][3][row]), count);
            }
            __syncthreads();
        }
        // ---- phase B: dres and dbranch, and the column sums of g * x^q and of g down the block ----
        take();
        const int which = (u >> 6) & 1, half = (u >> 5) & 1, ccol = 32 * (u >> 7) + (u & 31);   // the adding role: quantity, half of the rows, column
        const size_t r = kRows * b + lrow;
        const float rstd = wanted && r < rows ? a.rstd[r] : 0.0f;
        const float c1 = wanted ? c_s[0][lrow] : 0.0f, c2 = wanted ? c_s[1][lrow] : 0.0f;
        for (size_t round = 0; round < rounds; ++round) {
            const size_t tl = round * kGroups + grp, j0 = tl * kTileCols;
            const bool have = tl < across;
            const size_t cols = !have ? 0 : width - j0 < static_cast<size_t>(kTileCols) ? width - j0 : kTileCols;
            fetch(0, b, j0, cols);
            __syncthreads();
            if (have) {
                float xq[kBlock], up[kBlock], ghat[kBlock];
                piece(0, b, j0, cols, xq, up, ghat);
                if (mine != nullptr) {
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) {
                        tile[grp][0][tile_at(lrow, lcol + k)] = mul_rn(up[k], xq[k]);
                        tile[grp][1][tile_at(lrow, lcol + k)] = up[k];
                    }
                }
                if (wanted) {
                    const size_t col = j0 + lcol;
                    T rd[kBlock];
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) rd[k] = narrow<DT>(mul_rn(rstd, sub_rn(sub_rn(ghat[k], c1), mul_rn(xq[k], c2))));      // dx, as the plain kernel rounds it
                    if (gh != nullptr) {
                        T ra[kBlock];
                        load_piece<DT>(gh, a.ld_gh, a.vec_in, r, col, rows, width, ra);
#pragma unroll
                        for (int k = 0; k < kBlock; ++k) rd[k] = added<DT>(rd[k], ra[k]);
                    }
                    if (dres != nullptr) store_piece<DT>(dres, a.ld_dres, a.vec_out, r, col, rows, width, rd);
                    if (dbranch != nullptr) {
                        uint32_t w[4];
                        piece_mask(r, col, width, mask_key, a.threshold, w);
#pragma unroll
                        for (int k = 0; k < kBlock; ++k) rd[k] = dropped_gradient<DT>(rd[k], mask_bits(w, k) >= a.threshold, a.scale);
                        store_piece<DT>(dbranch, a.ld_dbranch, a.vec_out, r, col, rows, width, rd);
                    }
                }
            }
            __syncthreads();
            if (mine != nullptr) {                                              // (the whole workgroup alike: the exchange below takes every lane of a wave)
                const float *from = tile[grp][which];
                float sum = from[tile_at(kHalfRows * half, ccol)];
#pragma unroll 5
                for (int k = 1; k < kHalfRows; ++k) sum = add_rn(sum, from[tile_at(kHalfRows * half + k, ccol)]);
                const float other = __shfl_xor(sum, 32);                        // lanes 0 .. 31: rows 16 .. 31 of the same column
                if (half == 0 && static_cast<size_t>(ccol) < cols) {
                    const float total = add_rn(sum, other);
                    float *at = mine + which * width + j0 + ccol;
                    *at = first ? total : add_rn(*at, total);
                }
            }
            // (no barrier here: backward_kernel)
        }
    }
}

}  // namespace mxlnorm
}  // namespace quant
}  // namespace fewbit_hip

using namespace fewbit_hip::quant;
using fewbit_hip::sketch::key_of;

extern "C" {

size_t fewbit_hipx_mx_layer_norm_workspace(size_t rows, size_t width) { return mxlnorm::workspace_of(rows, width); }

int fewbit_hipx_mx_layer_norm_forward(int dtype, const void *x, size_t ld_x, size_t rows, size_t width, const void *gamma, const void *beta, float eps, int format,
                                      uint64_t seed, const uint64_t *seed_device, void *y, size_t ld_y, float *mean, float *rstd, uint8_t *cells,
                                      size_t cells_bytes, void *stream) {
    using namespace mxlnorm;
    const char *name = "mx_layer_norm_forward";
    if (const int rc = check_call(name, dtype, format, seed_device, rows, width)) return rc;
    if (x == nullptr || gamma == nullptr || y == nullptr || mean == nullptr || rstd == nullptr || cells == nullptr) return refuse_null(name);
    if (ld_x < width || ld_y < width)
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: a row stride ld (%zu, %zu) must be at least width = %zu", name, ld_x, ld_y, width);
    const size_t item = size_of(dtype);
    if (misaligned(x, item) || misaligned(y, item) || misaligned(gamma, item) || misaligned(beta, item) || misaligned(mean, sizeof(float)) ||
        misaligned(rstd, sizeof(float)))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: x, y, gamma, beta, mean and rstd must be aligned to their element size", name);
    if (const int rc = check_aligned16(name, "cells", cells)) return rc;
    if (const int rc = check_bytes(name, "cells", cells_bytes, fewbit_hip::mx::bytes_of(rows, width, format))) return rc;
    const size_t blocks = fewbit_hip::mx::blocks_of(rows);
    const ForwardArgs a{x, ld_x, rows, width, gamma, beta, eps, key_of(seed), reinterpret_cast<const Key *>(seed_device), y, ld_y, mean, rstd, cells, blocks,
                        wide(x, ld_x, dtype), wide(y, ld_y, dtype), wide(gamma, 0, dtype), wide(beta, 0, dtype)};
    const unsigned grid = static_cast<unsigned>(blocks < kMaxGridForward ? blocks : kMaxGridForward);
    pick_kernel(dtype, format, [&](auto dt, auto fmt) {
        hipLaunchKernelGGL((forward_kernel<dt(), fmt()>), dim3(grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

int fewbit_hipx_mx_layer_norm_backward(int dtype, const void *gy, size_t ld_gy, const uint8_t *cells, size_t cells_bytes, const float *rstd, const void *gamma,
                                       size_t rows, size_t width, int format, void *dx, size_t ld_dx, float *dgamma, float *dbeta, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    using namespace mxlnorm;
    const char *name = "mx_layer_norm_backward";
    const bool sums = dgamma != nullptr || dbeta != nullptr;
    if (const int rc = check_call(name, dtype, format, nullptr, rows, width)) return rc;
    if (gy == nullptr || cells == nullptr || rstd == nullptr || gamma == nullptr || (sums && workspace == nullptr)) return refuse_null(name);
    if (ld_gy < width || (dx != nullptr && ld_dx < width))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: a row stride ld (%zu, %zu) must be at least width = %zu", name, ld_gy, ld_dx, width);
    const size_t item = size_of(dtype);
    if (misaligned(gy, item) || misaligned(dx, item) || misaligned(gamma, item) || misaligned(rstd, sizeof(float)) || misaligned(dgamma, sizeof(float)) ||
        misaligned(dbeta, sizeof(float)) || misaligned(workspace, sizeof(float)))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: gy, dx, gamma, rstd, dgamma, dbeta and the workspace must be aligned to their element size", name);
    if (const int rc = check_aligned16(name, "cells", cells)) return rc;
    if (const int rc = check_bytes(name, "cells", cells_bytes, fewbit_hip::mx::bytes_of(rows, width, format))) return rc;
    if (sums)
        if (const int rc = check_bytes(name, "the workspace", workspace_bytes, workspace_of(rows, width))) return rc;
    if (dx == nullptr && !sums) return FEWBIT_OK;
    const size_t grid = backward_grid(rows);
    const BackwardArgs a{gy, ld_gy, cells, rstd, gamma, rows, width, dx, ld_dx, sums ? static_cast<float *>(workspace) : nullptr,
                         fewbit_hip::mx::blocks_of(rows), wide(gy, ld_gy, dtype), wide(dx, ld_dx, dtype), wide(gamma, 0, dtype)};
    pick_kernel(dtype, format, [&](auto dt, auto fmt) {
        hipLaunchKernelGGL((backward_kernel<dt(), fmt()>), dim3(static_cast<unsigned>(grid)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    });
    if (sums)
        hipLaunchKernelGGL(column_sums_kernel, dim3(static_cast<unsigned>((width + kTileCols - 1) / kTileCols), kSums), dim3(kThreads), 0,
                           static_cast<hipStream_t>(stream), static_cast<const float *>(workspace), grid, width, dgamma, dbeta);
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

int fewbit_hipx_mx_add_layer_norm_forward(int dtype, const void *x, size_t ld_x, const void *residual, size_t ld_residual, size_t rows, size_t width,
                                          const void *gamma, const void *beta, float eps, int format, uint64_t seed, uint64_t seed_mask,
                                          const uint64_t *seed_device, uint32_t threshold, void *y, size_t ld_y, void *h_out, size_t ld_h, float *mean,
                                          float *rstd, uint8_t *cells, size_t cells_bytes, void *stream) {
    using namespace mxlnorm;
    const char *name = "mx_add_layer_norm_forward";
    if (const int rc = check_call(name, dtype, format, seed_device, rows, width)) return rc;
    if (const int rc = check_mask(name, threshold, width)) return rc;
    if (residual == nullptr) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: null pointer (residual)", name);
    if (x == nullptr || gamma == nullptr || y == nullptr || rstd == nullptr || cells == nullptr) return refuse_null(name);
    if (ld_x < width || ld_residual < width || ld_y < width || (h_out != nullptr && ld_h < width))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: a row stride ld (%zu, %zu, %zu, %zu) must be at least width = %zu", name, ld_x, ld_residual, ld_y, ld_h, width);
    const size_t item = size_of(dtype);
    if (misaligned(x, item) || misaligned(residual, item) || misaligned(y, item) || misaligned(h_out, item) || misaligned(gamma, item) ||
        misaligned(beta, item) || misaligned(mean, sizeof(float)) || misaligned(rstd, sizeof(float)))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: x, residual, y, h_out, gamma, beta, mean and rstd must be aligned to their element size", name);
    if (const int rc = check_aligned16(name, "cells", cells)) return rc;
    if (const int rc = check_bytes(name, "cells", cells_bytes, fewbit_hip::mx::bytes_of(rows, width, format))) return rc;
    if (matrices_meet(y, ld_y, h_out, ld_h, rows, width, item)) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: y and h_out overlap", name);
    const size_t blocks = fewbit_hip::mx::blocks_of(rows);
    const AddForwardArgs a{x, residual, ld_x, ld_residual, rows, width, gamma, beta, eps, key_of(seed), key_of(seed_mask),
                           reinterpret_cast<const Key *>(seed_device), threshold, fewbit_hip::unit::scale_of(threshold), y, h_out, ld_y, ld_h, mean, rstd,
                           cells, blocks, wide(x, ld_x, dtype), wide(residual, ld_residual, dtype), wide(y, ld_y, dtype), wide(h_out, ld_h, dtype),
                           wide(gamma, 0, dtype), wide(beta, 0, dtype)};
    const unsigned grid = static_cast<unsigned>(blocks < kMaxGridForward ? blocks : kMaxGridForward);
    pick_kernel(dtype, format, [&](auto dt, auto fmt) {
        hipLaunchKernelGGL((add_forward_kernel<dt(), fmt()>), dim3(grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

int fewbit_hipx_mx_add_layer_norm_backward(int dtype, const void *gy, size_t ld_gy, const void *gy_add, size_t ld_gy_add, const void *gh, size_t ld_gh,
                                           const uint8_t *cells, size_t cells_bytes, const float *rstd, const void *gamma, size_t rows, size_t width,
                                           int format, uint64_t seed_mask, const uint64_t *seed_device, uint32_t threshold, void *dres, size_t ld_dres,
                                           void *dbranch, size_t ld_dbranch, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes,
                                           void *stream) {
    using namespace mxlnorm;
    const char *name = "mx_add_layer_norm_backward";
    const bool sums = dgamma != nullptr || dbeta != nullptr;
    if (const int rc = check_call(name, dtype, format, seed_device, rows, width)) return rc;
    if (const int rc = check_mask(name, threshold, width)) return rc;
    if (dbranch != nullptr && threshold == 0)
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: with threshold = 0 dbranch is dres: pass dbranch = NULL", name);
    if (gy == nullptr || cells == nullptr || rstd == nullptr || gamma == nullptr || (sums && workspace == nullptr)) return refuse_null(name);
    if (ld_gy < width || (gy_add != nullptr && ld_gy_add < width) || (gh != nullptr && ld_gh < width) || (dres != nullptr && ld_dres < width) ||
        (dbranch != nullptr && ld_dbranch < width))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: a row stride ld (%zu, %zu, %zu, %zu, %zu) must be at least width = %zu", name, ld_gy, ld_gy_add, ld_gh,
                    ld_dres, ld_dbranch, width);
    const size_t item = size_of(dtype);
    if (misaligned(gy, item) || misaligned(gy_add, item) || misaligned(gh, item) || misaligned(dres, item) || misaligned(dbranch, item) ||
        misaligned(gamma, item) || misaligned(rstd, sizeof(float)) || misaligned(dgamma, sizeof(float)) || misaligned(dbeta, sizeof(float)) ||
        misaligned(workspace, sizeof(float)))
        return fail(FEWBIT_ERR_INVALID_ARGUMENT,
                    "%s: gy, gy_add, gh, dres, dbranch, gamma, rstd, dgamma, dbeta and the workspace must be aligned to their element size", name);
    if (const int rc = check_aligned16(name, "cells", cells)) return rc;
    if (const int rc = check_bytes(name, "cells", cells_bytes, fewbit_hip::mx::bytes_of(rows, width, format))) return rc;
    if (sums)
        if (const int rc = check_bytes(name, "the workspace", workspace_bytes, workspace_of(rows, width))) return rc;
    if (matrices_meet(dres, ld_dres, dbranch, ld_dbranch, rows, width, item)) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: dres and dbranch overlap", name);
    if (dres == nullptr && dbranch == nullptr && !sums) return FEWBIT_OK;
    const size_t grid = backward_grid(rows);
    const AddBackwardArgs a{gy, gy_add, gh, ld_gy, ld_gy_add, ld_gh, cells, rstd, gamma, rows, width, key_of(seed_mask),
                            reinterpret_cast<const Key *>(seed_device), threshold, fewbit_hip::unit::scale_of(threshold), dres, dbranch, ld_dres, ld_dbranch,
                            sums ? static_cast<float *>(workspace) : nullptr, fewbit_hip::mx::blocks_of(rows),
                            wide(gy, ld_gy, dtype) && wide(gy_add, ld_gy_add, dtype) && wide(gh, ld_gh, dtype),
                            wide(dres, ld_dres, dtype) && wide(dbranch, ld_dbranch, dtype), wide(gamma, 0, dtype)};
    pick_kernel(dtype, format, [&](auto dt, auto fmt) {
        hipLaunchKernelGGL((add_backward_kernel<dt(), fmt()>), dim3(static_cast<unsigned>(grid)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    });
    if (sums)
        hipLaunchKernelGGL(column_sums_kernel, dim3(static_cast<unsigned>((width + kTileCols - 1) / kTileCols), kSums), dim3(kThreads), 0,
                           static_cast<hipStream_t>(stream), static_cast<const float *>(workspace), grid, width, dgamma, dbeta);
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

}  // extern "C"
