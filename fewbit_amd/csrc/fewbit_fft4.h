// fewbit_fft4.h -- the four-step fp32 FFT of the sampled transforms, shared by fewbit_dct.hip (sampled DCT-II) and fewbit_dft.hip
// (sampled DFT): tile constants, the small transforms in registers, the in-place LDS stages and their digit maps, the 16-byte row
// loads, the twiddle tables, the rows of a seed (RowsInMemory / RowsOfSeed) and their sort by residue class (sort_rows), the row
// split N = N1 x N2 (split_rows, FB_FFT4_SPLITS), the kernels of both passes (pass_a_kernel, pass_a_zext_kernel, pass_b_kernel), the
// workspace formula and the host side of a call (run: checks, LDS opt-in, dispatch).  The algorithm and the tiling are described in
// fewbit_dct.hip's header; the two transforms differ only in how pass A orders the rows it loads (RowsMakhoul / RowsInOrder) and in pass
// B's epilogue (CosineRows / FourierPlanes).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "fewbit_hip.h"
#include "fewbit_philox.h"
#include "fewbit_unit.h"

namespace fewbit_hip {
namespace dct {
constexpr int C = 32;                       // complex columns of a tile = 64 features
constexpr int kFeatures = 2 * C;
// Both passes: a 32 KiB tile + tables per 256-thread workgroup, four workgroups per CU, each in its own phase (loading, transforming,
// storing): pass A one row of transforms x 32 complex columns; pass B the two rows of a residue pair x 16 complex columns
constexpr int kThreadsA = 256, kRowsA = 1;
constexpr int kThreadsB = 256, CB = C / 2;  // pass B: 16 complex columns x the two rows of a residue pair
constexpr int kServeLanes = 4;              // pass B: lanes that write one sampled row (CB / kServeLanes complex columns each)

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

// complex product with two multiplies and two fused multiply-adds (the build has -ffp-contract=off: fusion is spelled out where wanted)
__device__ __forceinline__ f32x2 cmul(f32x2 a, f32x2 b) {
    return f32x2{__builtin_fmaf(a.x, b.x, -(a.y * b.y)), __builtin_fmaf(a.x, b.y, a.y * b.x)};
}
__device__ __forceinline__ f32x2 mul_mi(f32x2 a) { return f32x2{a.y, -a.x}; }                                   // a * (-i)
// e^{-2 pi i num / den}: den a power of two (num / den is exact in fp32), or 3, 5, 7, 9, 15 x a power of two (the angle in double, then rounded;
// `den` is a template constant at every call site: the branch folds)
__device__ __forceinline__ f32x2 unit(int num, int den) {
    if ((den & (den - 1)) != 0) {
        double s, c;
        sincospi(-2.0 * static_cast<double>(num) / static_cast<double>(den), &s, &c);
        return f32x2{static_cast<float>(c), static_cast<float>(s)};
    }
    float s, c;
    sincospif(-2.0f * static_cast<float>(num) / static_cast<float>(den), &s, &c);
    return f32x2{c, s};
}

// ---- small transforms in registers, natural order in and out: x[q] <- sum_j x[j] e^{-2 pi i j q / R} ------------------------------
constexpr float kR2 = 0.70710678118654752f;                   // sqrt(1/2)
constexpr float kC8 = 0.92387953251128674f, kS8 = 0.38268343236508977f;      // cos, sin of pi / 8
__device__ __forceinline__ void dft2(f32x2 &a, f32x2 &b) {
    const f32x2 s = a + b, d = a - b;
    a = s;
    b = d;
}
__device__ __forceinline__ void dft4(f32x2 &a0, f32x2 &a1, f32x2 &a2, f32x2 &a3) {
    const f32x2 t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3, t3 = mul_mi(a1 - a3);
    a0 = t0 + t2;
    a1 = t1 + t3;
    a2 = t0 - t2;
    a3 = t1 - t3;
}
constexpr float kH3 = 0.86602540378443865f;                   // sqrt(3) / 2
template <int R> __device__ __forceinline__ void dft(f32x2 (&x)[R]) {
    if constexpr (R == 2) {
        dft2(x[0], x[1]);
    } else if constexpr (R == 3) {
        // W3 = -1/2 - i sqrt(3)/2:  y1, y2 = x0 - (x1 + x2) / 2  +-  (-i) (sqrt(3) / 2) (x1 - x2)
        const f32x2 t = x[1] + x[2], d = mul_mi(x[1] - x[2]) * kH3, m = x[0] - t * 0.5f;
        x[0] = x[0] + t;
        x[1] = m + d;
        x[2] = m - d;
    } else if constexpr (R == 4) {
        dft4(x[0], x[1], x[2], x[3]);
    } else if constexpr (R == 5) {
        // W5^j = cos(2 pi j / 5) - i sin(2 pi j / 5):  y1, y4 = m1 -+ i n1,  y2, y3 = m2 -+ i n2
        constexpr float c1 = 0.30901699437494742f, c2 = -0.80901699437494742f, s1 = 0.95105651629515357f, s2 = 0.58778525229247313f;
        const f32x2 a1 = x[1] + x[4], a2 = x[2] + x[3], b1 = x[1] - x[4], b2 = x[2] - x[3];
        const f32x2 m1 = x[0] + a1 * c1 + a2 * c2, m2 = x[0] + a1 * c2 + a2 * c1;
        const f32x2 n1 = mul_mi(b1 * s1 + b2 * s2), n2 = mul_mi(b1 * s2 - b2 * s1);
        x[0] = x[0] + a1 + a2;
        x[1] = m1 + n1;
        x[4] = m1 - n1;
        x[2] = m2 + n2;
        x[3] = m2 - n2;
    } else if constexpr (R == 7) {
        // W7^j = cos(2 pi j / 7) - i sin(2 pi j / 7), a_j = x_j + x_{7-j}, b_j = x_j - x_{7-j}:  y_q, y_{7-q} = m_q -+ i n_q,
        // m_q = x0 + sum_j cos(2 pi j q / 7) a_j,  n_q = sum_j sin(2 pi j q / 7) b_j
        constexpr float c1 = 0.62348980185873353f, c2 = -0.22252093395631440f, c3 = -0.90096886790241913f;
        constexpr float s1 = 0.78183148246802981f, s2 = 0.97492791218182361f, s3 = 0.43388373911755812f;
        const f32x2 a1 = x[1] + x[6], a2 = x[2] + x[5], a3 = x[3] + x[4], b1 = x[1] - x[6], b2 = x[2] - x[5], b3 = x[3] - x[4];
        const f32x2 m1 = x[0] + a1 * c1 + a2 * c2 + a3 * c3, m2 = x[0] + a1 * c2 + a2 * c3 + a3 * c1, m3 = x[0] + a1 * c3 + a2 * c1 + a3 * c2;
        const f32x2 n1 = mul_mi(b1 * s1 + b2 * s2 + b3 * s3), n2 = mul_mi(b1 * s2 - b2 * s3 - b3 * s1), n3 = mul_mi(b1 * s3 - b2 * s1 + b3 * s2);
        x[0] = x[0] + a1 + a2 + a3;
        x[1] = m1 + n1;
        x[6] = m1 - n1;
        x[2] = m2 + n2;
        x[5] = m2 - n2;
        x[3] = m3 + n3;
        x[4] = m3 - n3;
    } else if constexpr (R == 8) {
        // j = 2a + b, q = p + 4 q':  y[p + 4 q'] = sum_b W8^{bp} (-1)^{b q'} sum_a x[2a + b] W4^{ap}
        dft4(x[0], x[2], x[4], x[6]);
        dft4(x[1], x[3], x[5], x[7]);
        const f32x2 u1 = x[3], u2 = x[5], u3 = x[7];
        const f32x2 t0 = x[1];
        const f32x2 t1 = f32x2{(u1.x + u1.y) * kR2, (u1.y - u1.x) * kR2};             // * W8^1 = sqrt(1/2) (1 - i)
        const f32x2 t2 = mul_mi(u2);                                                   // * W8^2
        const f32x2 t3 = f32x2{(u3.y - u3.x) * kR2, -(u3.x + u3.y) * kR2};            // * W8^3 = -sqrt(1/2) (1 + i)
        const f32x2 e0 = x[0], e1 = x[2], e2 = x[4], e3 = x[6];
        x[0] = e0 + t0; x[4] = e0 - t0;
        x[1] = e1 + t1; x[5] = e1 - t1;
        x[2] = e2 + t2; x[6] = e2 - t2;
        x[3] = e3 + t3; x[7] = e3 - t3;
    } else {
        static_assert(R == 16, "radix 2, 3, 4, 5, 7, 8 or 16");
        // j = 4a + b, q = p + 4 q':  y[p + 4 q'] = sum_b W16^{bp} W4^{b q'} sum_a x[4a + b] W4^{ap}
        dft4(x[0], x[4], x[8], x[12]);
        dft4(x[1], x[5], x[9], x[13]);
        dft4(x[2], x[6], x[10], x[14]);
        dft4(x[3], x[7], x[11], x[15]);
        // u[b][p] = x[4p + b]; twiddle W16^{bp}
        x[5] = cmul(x[5], f32x2{kC8, -kS8});                                           // b = 1, p = 1: W16^1
        x[9] = f32x2{(x[9].x + x[9].y) * kR2, (x[9].y - x[9].x) * kR2};               // b = 1, p = 2: W16^2 = W8^1
        x[13] = cmul(x[13], f32x2{kS8, -kC8});                                         // b = 1, p = 3: W16^3
        x[6] = f32x2{(x[6].x + x[6].y) * kR2, (x[6].y - x[6].x) * kR2};               // b = 2, p = 1: W16^2
        x[10] = mul_mi(x[10]);                                                         // b = 2, p = 2: W16^4 = -i
        x[14] = f32x2{(x[14].y - x[14].x) * kR2, -(x[14].x + x[14].y) * kR2};         // b = 2, p = 3: W16^6 = W8^3
        x[7] = cmul(x[7], f32x2{kS8, -kC8});                                           // b = 3, p = 1: W16^3
        x[11] = f32x2{(x[11].y - x[11].x) * kR2, -(x[11].x + x[11].y) * kR2};         // b = 3, p = 2: W16^6
        x[15] = cmul(x[15], f32x2{-kC8, kS8});                                         // b = 3, p = 3: W16^9
        // outer transforms over b for each p; result q' of group p is output p + 4 q' -- which is where dft4 leaves it when the
        // group is (x[4p], x[4p+1], x[4p+2], x[4p+3]) and the outputs are then transposed: y[p + 4q'] = group_p[q']
        dft4(x[0], x[1], x[2], x[3]);
        dft4(x[4], x[5], x[6], x[7]);
        dft4(x[8], x[9], x[10], x[11]);
        dft4(x[12], x[13], x[14], x[15]);
        f32x2 y[16];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) y[p + 4 * q] = x[4 * p + q];
#pragma unroll
        for (int q = 0; q < 16; ++q) x[q] = y[q];
    }
}

// radix of the first stage of a block of length `len`: 256 = 16 x 16, 128 = 16 x 8, 64 = 8 x 8, 32 = 8 x 4, 16 = 16; a factor 3
// (48 = 3 x 16, 96 = 3 x 8 x 4, 192 = 3 x 8 x 8), 5 (80 = 5 x 16, 160 = 5 x 8 x 4) or 7 (112 = 7 x 16, 224 = 7 x 8 x 4) goes first, threes
// before a five (144 = 3 x 3 x 16, 288 = 3 x 3 x 8 x 4, 240 = 3 x 5 x 16)
__host__ __device__ constexpr int first_radix(int len) {
    return len % 3 == 0 ? 3 : len % 5 == 0 ? 5 : len % 7 == 0 ? 7 : len >= 128 ? 16 : len == 64 ? 8 : len == 32 ? 8 : len == 16 ? 16 : len == 8 ? 8 : len == 4 ? 4 : 2;
}

// position P (after the in-place DIF stages) -> frequency k.  Stage i with radix r_i on blocks of length L_i leaves digit q_i
// (k = q_1 + r_1 q_2 + r_1 r_2 q_3 + ...) in sub-block q_i: P = sum q_i L_i / r_i.
template <int LEN> __host__ __device__ __forceinline__ int pos_to_freq(int p) {
    if constexpr (LEN <= 1) {
        return 0;
    } else {
        constexpr int r = first_radix(LEN), s = LEN / r;
        return p / s + r * pos_to_freq<s>(p % s);
    }
}
template <int LEN> __host__ __device__ __forceinline__ int freq_to_pos(int k) {
    if constexpr (LEN <= 1) {
        return 0;
    } else {
        constexpr int r = first_radix(LEN), s = LEN / r;
        return (k % r) * s + freq_to_pos<s>(k / r);
    }
}

// One stage of the in-place transform of the tile [TR][L][C] along its middle axis: blocks of length LEN, radix R, twiddles
// tw[m] = W_L^m.  Thread (c = tid % 32, slot = tid / 32 of SLOTS) takes the butterflies slot, slot + SLOTS, ... of column c of all
// TR rows; a butterfly is R loads, the transform in registers, the twiddles W_LEN^{ss q} (none in the last stage) and R stores.
template <int L, int LEN, int R, int TR, int SLOTS> __device__ __forceinline__ void stage(f32x2 *tile, const f32x2 *tw, int c, int slot) {
    constexpr int S = LEN / R, kPerRow = L / R;
#pragma unroll
    for (int bid0 = 0; bid0 < TR * kPerRow; bid0 += SLOTS) {
        const int bid = bid0 + slot;
        if (TR * kPerRow % SLOTS != 0 && bid >= TR * kPerRow) break;
        const int row = bid / kPerRow, b = bid % kPerRow, block = b / S, ss = b % S;
        f32x2 *p = tile + (row * L + block * LEN + ss) * C + c;
        f32x2 x[R];
#pragma unroll
        for (int j = 0; j < R; ++j) x[j] = p[j * S * C];
        dft<R>(x);
        if constexpr (S > 1) {
#pragma unroll
            for (int q = 1; q < R; ++q) x[q] = cmul(x[q], tw[(L / LEN) * ss * q]);
        }
#pragma unroll
        for (int q = 0; q < R; ++q) p[q * S * C] = x[q];
    }
    __syncthreads();
}

template <int L, int TR, int SLOTS, int LEN = L> __device__ __forceinline__ void fft_tile(f32x2 *tile, const f32x2 *tw, int c, int slot) {
    if constexpr (LEN > 1) {
        constexpr int R = first_radix(LEN);
        stage<L, LEN, R, TR, SLOTS>(tile, tw, c, slot);
        fft_tile<L, TR, SLOTS, LEN / R>(tile, tw, c, slot);
    }
}

template <int DT> struct In {             // 16-byte piece of a row: 8 features of a 16-bit dtype, 4 of fp32
    static constexpr int kPieceFeatures = DT == FEWBIT_F32 ? 4 : 8;
    static constexpr int kPiecesPerSegment = kFeatures / kPieceFeatures;
};

__device__ __forceinline__ float half_to_float(uint32_t h, int dt) {
    if (dt == FEWBIT_BF16) return __builtin_bit_cast(float, h << 16);
    return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(h)));
}

// the piece `piece` of the 64-feature segment of row `row` that starts at feature f0, raw (16 bytes: 8 features of a 16-bit dtype or
// 4 of fp32).  FULL: the whole tile lies inside the matrix (a workgroup-uniform fact): one unguarded 16-byte load -- a load under a
// lane-divergent guard makes hipcc wait for it on the spot, which serialised the tile's loads; otherwise zeros beyond `features`,
// element by element.  The conversion to fp32 happens when the piece is written to LDS (unpack), after the latency has been used.
template <int DT, bool FULL> __device__ __forceinline__ u32x4 load_piece(const void *x, size_t row, size_t ld, size_t f0, int piece, size_t features) {
    constexpr int PF = In<DT>::kPieceFeatures;
    const size_t f = f0 + static_cast<size_t>(piece) * PF;
    if constexpr (DT == FEWBIT_F32) {
        const uint32_t *p = static_cast<const uint32_t *>(x) + row * ld + f;
        if (FULL || f + PF <= features) {
            typedef u32x4 __attribute__((aligned(4))) u32x4u;
            return *reinterpret_cast<const u32x4u *>(p);
        }
        u32x4 q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = f + e < features ? p[e] : 0u;
        return q;
    } else {
        const uint16_t *p = static_cast<const uint16_t *>(x) + row * ld + f;
        if (FULL || f + PF <= features) {
            typedef u32x4 __attribute__((aligned(2))) u32x4u;
            return *reinterpret_cast<const u32x4u *>(p);
        }
        u32x4 q = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e >> 1] |= (f + e < features ? static_cast<uint32_t>(p[e]) : 0u) << (16 * (e & 1));
        return q;
    }
}
template <int DT> __device__ __forceinline__ void unpack_piece(u32x4 q, float (&v)[In<DT>::kPieceFeatures]) {
    if constexpr (DT == FEWBIT_F32) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t w = q[e];              // (a scalar first: __builtin_bit_cast applied to the element expression q[e] itself
            v[e] = __builtin_bit_cast(float, w);  //  reads the vector's first element for every e -- observed with hipcc 7.2)
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[2 * e] = half_to_float(q[e] & 0xffffu, DT);
            v[2 * e + 1] = half_to_float(q[e] >> 16, DT);
        }
    }
}

// 2 E values of a result row (or of one plane of it) at element `at` of `out` (features fa .. fa + 2 E of the row): pass B's vector stores,
// element by element where the row ends inside them
template <int ODT, int E>
__device__ __forceinline__ void store_values(void *out, size_t at, const float (&y)[2 * E], size_t fa, size_t features) {
    if constexpr (ODT == FEWBIT_F32) {
        float *o = static_cast<float *>(out) + at;
        if (fa + 2 * E <= features) {
            if constexpr (E == 1) {
                *reinterpret_cast<f32x2 *>(o) = f32x2{y[0], y[1]};
            } else {
                typedef f32x4 __attribute__((aligned(4))) f32x4u;
#pragma unroll
                for (int e = 0; e < E; e += 2) *reinterpret_cast<f32x4u *>(o + 2 * e) = f32x4{y[2 * e], y[2 * e + 1], y[2 * e + 2], y[2 * e + 3]};
            }
        } else {
#pragma unroll
            for (int e = 0; e < 2 * E; ++e) if (fa + e < features) o[e] = y[e];
        }
    } else {
        uint16_t *o = static_cast<uint16_t *>(out) + at;
        uint16_t h[2 * E];
#pragma unroll
        for (int e = 0; e < 2 * E; ++e) {
            if constexpr (ODT == FEWBIT_BF16) h[e] = __builtin_bit_cast(uint16_t, static_cast<__bf16>(y[e]));
            else h[e] = __builtin_bit_cast(uint16_t, static_cast<_Float16>(y[e]));
        }
        if (fa + 2 * E <= features) {
            typedef uint32_t __attribute__((aligned(2))) u32u;
            typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
            typedef u32x2 __attribute__((aligned(2))) u32x2u;
            typedef u32x4 __attribute__((aligned(2))) u32x4u;
            auto pair = [&](int e) -> uint32_t { return static_cast<uint32_t>(h[2 * e]) | (static_cast<uint32_t>(h[2 * e + 1]) << 16); };
            if constexpr (E == 1) *reinterpret_cast<u32u *>(o) = pair(0);
            else if constexpr (E == 2) *reinterpret_cast<u32x2u *>(o) = u32x2{pair(0), pair(1)};
            else *reinterpret_cast<u32x4u *>(o) = u32x4{pair(0), pair(1), pair(2), pair(3)};
        } else {
#pragma unroll
            for (int e = 0; e < 2 * E; ++e) if (fa + e < features) o[e] = h[e];
        }
    }
}

constexpr int kFine = 128;                  // W_D^e = fine[e % 128] * coarse[e / 128] for e < N (coarse: N / 128 entries, at most 2048)
constexpr int coarse_entries(int n) { return n / kFine > 0 ? n / kFine : 1; }
__device__ __forceinline__ f32x2 table_unit(const f32x2 *fine, const f32x2 *coarse, int e, bool has_coarse) {
    return has_coarse ? cmul(fine[e % kFine], coarse[e / kFine]) : fine[e % kFine];
}

// ---- the sampled rows ------------------------------------------------------------------------------------------------------------
// Where they come from.  RowsInMemory: the caller's int64 array.  RowsOfSeed: a FUNCTION of a 64-bit seed,
//     rows = 2^k:      idx[j] = 16-bit half j % 8 of the 128 bits of Philox4x32-10(counter = (j / 8, 0, 0, 3), key = seed)  mod  rows
//                      (half h = bits 16 (h % 2) .. 16 (h % 2) + 15 of word h / 2)
//     any other rows:  idx[j] = (word j % 4 of Philox4x32-10(counter = (j / 4, 0, 0, 3), key = seed)  x  rows)  >>  32
// (uniform -- in the second case up to rows / 2^32 --, with replacement, like the reference's T.multinomial of equal weights): no array, no
// launch that draws one, nothing to keep for backward but the seed -- and, with the seed read from device memory, a recorded launch draws
// fresh rows on every replay (fewbit_sketch.hip, same scheme).
constexpr uint32_t kRowsDomain = 3u;        // counter word 3 (0 and 2: the dense sketches)
__host__ __device__ constexpr bool power_of_two(size_t n) { return (n & (n - 1)) == 0; }
// rows = 2^k <= 2^16: eight 16-bit halves per Philox call; any other row count (3, 5, 7, 9, 15 x 2^k, 2^17, 2^18): four 32-bit words, word x rows >> 32
__host__ __device__ constexpr bool draws_halves(size_t n) { return power_of_two(n) && n <= 65536; }
__host__ __device__ constexpr int per_draw(bool halves) { return halves ? 8 : 4; }      // row numbers per Philox call
// row number h of one Philox call (HALVES: not yet reduced mod rows -- the caller masks)
template <bool HALVES> __host__ __device__ __forceinline__ int drawn_row(const uint32_t (&w)[4], int h, uint32_t rows) {
    if constexpr (HALVES) return static_cast<int>((w[h / 2] >> (16 * (h % 2))) & 0xffffu);
    else return static_cast<int>((static_cast<uint64_t>(w[h]) * rows) >> 32);
}
struct RowsInMemory {
    static constexpr bool kSeeded = false, kSigned = false;
    const int64_t *idx;
};
struct RowsOfSeed {
    static constexpr bool kSeeded = true, kSigned = false;
    sketch::Key value;
    const sketch::Key *device;              // != nullptr: the key is read from there when the kernel runs
};
// The rows of a seed AND its signs: the matrix is transformed as D m, D = diag(+-1) a function of the same seed (the random diagonal of
// a subsampled randomized Fourier transform: it flattens the row energies of T D m whatever the rows of m share).
//     w[0..3] = Philox4x32-10(counter = (low 32 bits of r >> 7, high 32 bits of r >> 7, 0, 6), key = seed)
//     flip(r) = bit (r & 31) of w[(r >> 5) & 3]          1: row r of m (as it lies in memory) is negated
// Only pass_a_zext_kernel knows it (ROWS::kSigned); the sampled rows and their sort are RowsOfSeed's.  The flag is a constant of the ROWS
// type and not a template parameter of the kernel: a sixth parameter would rename every existing instantiation, and the kernels keep their
// names and their machine code (tools/isa_digest.py --diff: profiles/signed_transform_isa_identity.txt).
constexpr uint32_t kSignsDomain = 6u;       // counter word 3 (4: the CRS columns, 5: dropout)
struct SignedRowsOfSeed : RowsOfSeed {
    static constexpr bool kSigned = true;
};
__host__ __device__ __forceinline__ bool row_flipped(sketch::Key key, uint64_t r) {
    const uint64_t q = r >> 7;
    uint32_t w[4];
    sketch::philox4x32(static_cast<uint32_t>(q), static_cast<uint32_t>(q >> 32), 0u, kSignsDomain, key, w);
    return ((w[(r >> 5) & 3] >> (r & 31)) & 1u) != 0u;
}

// Pass B's workgroup (u, t) writes the samples k with k % N1 in {u, N1 - u}.  So that its 24 .. 96 siblings (one per half tile) need
// not each test all of idx -- a third of pass B's time when they did (profiles/r06_dct_variants.txt: "noenlist") -- ONE workgroup, pass
// A's (0, 0) before it turns to its own tile, sorts the samples by u into the workspace:
//     sorted[offsets[u] .. offsets[u + 1])  =  the samples (k, j) with min(k % N1, N1 - k % N1) = u,   u = 0 .. N1 / 2
// A counting sort in LDS: histogram, prefix, placement.  The order inside a class is whatever the atomics give; no result depends on it
// (every sample writes its own row of the output).
struct Sample { int k, j; };                // frequency, row of the output
constexpr size_t kOffsetsBytes = 2048;      // (N1 / 2 + 2 ints, N1 <= 512, rounded up)

template <int N1, int N, typename ROWS>
__device__ __forceinline__ void sort_rows(ROWS rows, size_t proj, int *__restrict__ offsets, Sample *__restrict__ sorted, int *lds, int tid) {
    constexpr int U = N1 / 2 + 1, kThreads = kThreadsA;
    constexpr bool kPow2 = power_of_two(N), kHalves = draws_halves(N);
    constexpr int kPerDraw = per_draw(kHalves);
    int *hist = lds, *cursor = lds + U + 1;
    sketch::Key key{0u, 0u};
    if constexpr (ROWS::kSeeded) {
        key = rows.value;
        if (rows.device != nullptr) key = *rows.device;               // (one scalar load)
    }
    auto bucket = [](int k) -> int {
        const int k1 = k % N1;
        return k1 <= N1 / 2 ? k1 : N1 - k1;
    };
    // every (k, j) this thread looks after: of an array j = tid, tid + 256, ...; of a seed the numbers of the Philox calls tid, tid + 256, ...
    auto for_each = [&](auto &&f) __attribute__((always_inline)) {
        if constexpr (ROWS::kSeeded) {
            for (size_t q = tid; kPerDraw * q < proj; q += kThreads) {
                uint32_t w[4];
                sketch::philox4x32(static_cast<uint32_t>(q), static_cast<uint32_t>(q >> 32), 0u, kRowsDomain, key, w);
#pragma unroll
                for (int h = 0; h < kPerDraw; ++h) {
                    const size_t j = kPerDraw * q + h;
                    const int drawn = drawn_row<kHalves>(w, h, N);
                    if (j < proj) f(kHalves ? drawn & (N - 1) : drawn, j);
                }
            }
        } else {
            // (the low dword of an int64 in [0, N) is the number; whatever else the array holds is reduced to [0, N))
            // eight unconditional requests (a clamped index) before the first is looked at: eight latencies overlap instead of following one another
            const int *lo = reinterpret_cast<const int *>(rows.idx);
            for (size_t j0 = tid; j0 < proj; j0 += 8 * kThreads) {
                int word[8];
#pragma unroll
                for (int a = 0; a < 8; ++a) {
                    const size_t j = j0 + static_cast<size_t>(a) * kThreads;
                    word[a] = lo[2 * (j < proj ? j : proj - 1)];
                }
#pragma unroll
                for (int a = 0; a < 8; ++a) {
                    const size_t j = j0 + static_cast<size_t>(a) * kThreads;
                    if (j < proj) f(kPow2 ? word[a] & (N - 1) : static_cast<int>(static_cast<unsigned>(word[a]) % static_cast<unsigned>(N)), j);
                }
            }
        }
    };
    for (int b = tid; b <= U; b += kThreads) hist[b] = 0;
    __syncthreads();
    for_each([&](int k, size_t) { atomicAdd(&hist[bucket(k)], 1); });
    __syncthreads();
    for (int mine = tid; mine <= U; mine += kThreads) {                // offsets[b] = the classes before b (every lane reads the same word: a broadcast)
        int run = 0;
#pragma unroll 8
        for (int b = 0; b < U; ++b) {
            const int n = hist[b];
            run += b < mine ? n : 0;
        }
        cursor[mine] = run;
        offsets[mine] = run;
    }
    __syncthreads();
    for_each([&](int k, size_t j) {
        const int pos = atomicAdd(&cursor[bucket(k)], 1);
        sorted[pos] = Sample{k, static_cast<int>(j)};
    });
    __syncthreads();                                                   // (the tile takes this LDS over)
}

// ---- pass A -----------------------------------------------------------------------------------------------------------------
// ORDER says which row of the matrix the point n of the transformed sequence is: the DFT's is row n, the DCT's Makhoul's reordering
// (fewbit_dct.hip, step 1).  kReordered is what pass_a_kernel reads, row<N>(n) what pass_a_zext_kernel calls: the same map twice.
struct RowsInOrder {
    static constexpr bool kReordered = false;
    template <int N> static __device__ __forceinline__ size_t row(int n) { return static_cast<size_t>(n); }
};
struct RowsMakhoul {
    static constexpr bool kReordered = true;
    template <int N> static __device__ __forceinline__ size_t row(int n) { return n < N / 2 ? 2 * static_cast<size_t>(n) : 2 * static_cast<size_t>(N - 1 - n) + 1; }
};
// grid (N2, column tiles): workgroup (b, t) transforms the rows n = N2 n1 + b of column tile t.  inter: [half tile][k1][n2][16] complex fp32.
// (One text for both transforms as a KERNEL template, not as an inlined function that two kernels call: a shared __forceinline__ body
// gave 34 of the 152 bf16 kernels another machine code -- other instructions from N1 = 256 on -- while this template, with the row
// spelled here under ORDER::kReordered and not taken through ORDER::row<N>, which reorders the DCT's 16-bit N1 = 16 kernels, compiles to the
// instructions the two former kernels had: EXPERIMENTS 8.16.)
template <typename ORDER, int DT, int N1, int N2, typename ROWS>
__global__ __launch_bounds__(kThreadsA, (N1 > 128 ? 2 : 4)) void pass_a_kernel(const void *__restrict__ x, size_t features, size_t ld, f32x2 *__restrict__ inter, ROWS rows,
                                                              size_t proj, int *__restrict__ offsets, Sample *__restrict__ sorted) {
    constexpr int N = N1 * N2, kCoarse = coarse_entries(N), kThreads = kThreadsA, kSlots = kThreads / C;
    static_assert(kRowsA == 1, "one n2 per workgroup");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    f32x2 *tile = reinterpret_cast<f32x2 *>(lds_raw);                 // [N1][C]
    f32x2 *tw = tile + N1 * C;                                        // W_N1^m, m < N1
    f32x2 *fine = tw + N1, *coarse = fine + kFine;                    // W_N^m (m < 128), W_N^{128 m}
    const int tid = threadIdx.x, c = tid % C, slot = tid / C;
    const int b = blockIdx.x;
    const size_t t = blockIdx.y, f0 = t * kFeatures;
    // one workgroup of the launch sorts the sampled rows for pass B first (~2 us of its own time; the launch takes 16)
    if (blockIdx.x == 0 && blockIdx.y == 0) sort_rows<N1, N, ROWS>(rows, proj, offsets, sorted, reinterpret_cast<int *>(lds_raw), tid);

    // ---- loads first (all in flight), tables while they travel, then registers -> LDS
    constexpr int PF = In<DT>::kPieceFeatures, PPS = In<DT>::kPiecesPerSegment, kTotal = N1 * PPS, kPieces = (kTotal + kThreads - 1) / kThreads;
    // (one body per case, FULL tile or edge tile, each with its own registers from the loads to the LDS writes: were the two
    // cases to meet in one set of registers in between, the copies at the join would wait for the loads right behind their issue)
    auto fill_tile = [&](auto full) __attribute__((always_inline)) {
        u32x4 raw[kPieces];
#pragma unroll
        for (int i = 0; i < kPieces; ++i) {
            const int pid = tid + kThreads * i, n1 = pid / PPS, piece = pid % PPS;
            if (kTotal % kThreads != 0 && pid >= kTotal) break;
            const int n = N2 * n1 + b;                                  // index into the transformed sequence (the DCT's: the reordered v)
            const size_t row = ORDER::kReordered ? (n < N / 2 ? 2 * static_cast<size_t>(n) : 2 * static_cast<size_t>(N - 1 - n) + 1) : static_cast<size_t>(n);
            raw[i] = load_piece<DT, decltype(full)::value>(x, row, ld, f0, piece, features);
        }
        for (int m = tid; m < N1; m += kThreads) tw[m] = unit(m, N1);
        for (int m = tid; m < kFine; m += kThreads) fine[m] = unit(m, N);
        for (int m = tid; m < kCoarse; m += kThreads) coarse[m] = unit(m * kFine, N);
#pragma unroll
        for (int i = 0; i < kPieces; ++i) {
            const int pid = tid + kThreads * i, n1 = pid / PPS, piece = pid % PPS;
            if (kTotal % kThreads != 0 && pid >= kTotal) break;
            float v[PF];
            unpack_piece<DT>(raw[i], v);
            f32x4 *dst = reinterpret_cast<f32x4 *>(tile + n1 * C + piece * (PF / 2));
#pragma unroll
            for (int e = 0; e < PF / 4; ++e) dst[e] = f32x4{v[4 * e], v[4 * e + 1], v[4 * e + 2], v[4 * e + 3]};
        }
    };
    if (f0 + kFeatures <= features) fill_tile(std::true_type{});       // (workgroup-uniform)
    else fill_tile(std::false_type{});
    __syncthreads();

    fft_tile<N1, kRowsA, kSlots>(tile, tw, c, slot);

    // ---- twiddle + store: unit = two complex columns (16 B) of one position P; 16 consecutive lanes = the 256 contiguous bytes of one k1
    constexpr int kUnitsTotal = N1 * (C / 2), kUnits = (kUnitsTotal + kThreads - 1) / kThreads;
#pragma unroll
    for (int i = 0; i < kUnits; ++i) {
        const int uid = tid + kThreads * i, c2 = uid % (C / 2), p = uid / (C / 2);
        if (kUnitsTotal % kThreads != 0 && uid >= kUnitsTotal) break;
        const int k1 = pos_to_freq<N1>(p), e = b * k1;
        const f32x2 w = table_unit(fine, coarse, e, kCoarse > 1);
        const f32x4 z = *reinterpret_cast<const f32x4 *>(tile + p * C + 2 * c2);
        const f32x2 a = cmul(f32x2{z[0], z[1]}, w), bb = cmul(f32x2{z[2], z[3]}, w);
        // (the intermediate is kept per HALF tile of 16 complex columns -- what one pass-B workgroup reads: 128 contiguous bytes here)
        f32x4 *dst = reinterpret_cast<f32x4 *>(inter + (((2 * t + c2 / (CB / 2)) * N1 + k1) * N2 + b) * CB + 2 * (c2 % (CB / 2)));
        *dst = f32x4{a.x, a.y, bb.x, bb.y};
    }
}

// ---- pass A of a zero-extended call ---------------------------------------------------------------------------------------------
// The matrix has valid_rows <= N rows in memory and counts as N rows, the missing ones zero.
// pass_a_kernel (the algorithm, the tile, the intermediate) with ONE difference: a 16-byte piece whose row is >= valid_rows is zeros in
// registers and no memory request is made for it, so nothing at or beyond row valid_rows of x is read and the pass moves valid_rows / N
// of the bytes.  Everything after the tile is filled is the same arithmetic on the same values as the plain kernel's on a zero-filled
// copy: the same bits.
// WHICH COPY LEADS.  Pass A exists twice: pass_a_kernel and this one.  The plain kernel is the authoritative text: a change to pass A is
// made there first and then repeated here line by line (the bit-equality test of tests/test_gpu_transform_zext.py fails when this copy
// is left behind).  Why the two are not one.  (1) Folded into pass_a_kernel through a span type as second kernel parameter, empty for
// the plain kernels, this text changes the machine code of all 152 plain bf16 kernels (the instruction counts stay, the kernel-argument
// offsets move) and of 90 of the 228 zero-extended and signed ones, and the project keeps measured kernels instruction for instruction
// (EXPERIMENTS 8.16).  (2) Nor can the plain path become valid_rows = N of this kernel: it reaches the full tiles through a buffer
// descriptor whose size is 32 bits (below), while the plain kernels, on 64-bit addresses, take matrices that span 4 GiB and more.
// How a piece is left out.  A load under a lane-divergent `if (row < valid_rows)` makes hipcc wait for each load where the branches join
// (the tile's loads then follow one another: seen in the assembly of this kernel written that way).  So the pieces of a full tile are
// buffer loads through a descriptor of the valid_rows x ld elements of x: a piece of a missing row is given the offset kBeyondZext, which
// the hardware's range check (offset >= the descriptor's bytes) answers with zeros without a memory access -- no branch, all loads in
// flight at once as in the plain kernel.  The descriptor's size is 32 bits: valid_rows x ld elements must be below 4 GiB (zext_span_ok;
// the host refuses more).  The edge tile (features % 64 != 0), loaded element by element as in the plain kernel, keeps the `if`.
// The signs of a seed (ROWS = SignedRowsOfSeed; every other ROWS compiles to the code it was).  While its loads travel, the workgroup
// evaluates flip(row) of the N1 rows it touches ONCE (at most two Philox calls per thread) into a table at the start of the tile's LDS,
// every thread takes the entries of its own pieces into registers, and the tile is filled as before with ONE difference: the raw piece
// is XORed with the sign bits of its elements (0x80008000 / 0x80000000 per dword) before it is unpacked -- exact in all three dtypes, the
// bits of a matrix negated in memory.  Only what was loaded is flipped: a missing row and the zeros behind `features` in the edge tile
// stay +0, so the result is bit for bit the unsigned kernel's on m with the flipped rows negated.  No branch around a load; the two
// barriers stand between the loads' issue and their first use.
constexpr uint32_t kBeyondZext = 0xfffffff0u;
// the sign bits of the elements of a 16-byte piece that starts at feature f and lie inside the row (the whole piece in a full tile)
template <int DT, bool FULL> __device__ __forceinline__ u32x4 sign_bits(size_t f, size_t features) {
    if constexpr (DT == FEWBIT_F32) {
        if (FULL || f + 4 <= features) return u32x4{0x80000000u, 0x80000000u, 0x80000000u, 0x80000000u};
        u32x4 q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = f + e < features ? 0x80000000u : 0u;
        return q;
    } else {
        if (FULL || f + 8 <= features) return u32x4{0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u};
        u32x4 q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = (f + 2 * e < features ? 0x8000u : 0u) | (f + 2 * e + 1 < features ? 0x80000000u : 0u);
        return q;
    }
}
inline bool zext_span_ok(size_t valid_rows, size_t ld, int dtype) {
    const size_t row_bytes = ld * (dtype == FEWBIT_F32 ? 4 : 2);
    return row_bytes == 0 || valid_rows <= static_cast<size_t>(kBeyondZext) / row_bytes;
}
template <typename ORDER, int DT, int N1, int N2, typename ROWS>
__global__ __launch_bounds__(kThreadsA, (N1 > 128 ? 2 : 4)) void pass_a_zext_kernel(const void *__restrict__ x, size_t valid_rows, size_t features, size_t ld,
                                                                   f32x2 *__restrict__ inter, ROWS rows, size_t proj, int *__restrict__ offsets,
                                                                   Sample *__restrict__ sorted) {
    constexpr int N = N1 * N2, kCoarse = coarse_entries(N), kThreads = kThreadsA, kSlots = kThreads / C;
    static_assert(kRowsA == 1, "one n2 per workgroup");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    f32x2 *tile = reinterpret_cast<f32x2 *>(lds_raw);                 // [N1][C]
    f32x2 *tw = tile + N1 * C;                                        // W_N1^m, m < N1
    f32x2 *fine = tw + N1, *coarse = fine + kFine;                    // W_N^m (m < 128), W_N^{128 m}
    const int tid = threadIdx.x, c = tid % C, slot = tid / C;
    const int b = blockIdx.x;
    const size_t t = blockIdx.y, f0 = t * kFeatures;
    if (blockIdx.x == 0 && blockIdx.y == 0) sort_rows<N1, N, ROWS>(rows, proj, offsets, sorted, reinterpret_cast<int *>(lds_raw), tid);

    constexpr int PF = In<DT>::kPieceFeatures, PPS = In<DT>::kPiecesPerSegment, kTotal = N1 * PPS, kPieces = (kTotal + kThreads - 1) / kThreads;
    constexpr size_t kElementBytes = DT == FEWBIT_F32 ? 4 : 2;
    // the rows of x that exist (built from kernel arguments only: uniform)
    const __amdgpu_buffer_rsrc_t held = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(x), 0, static_cast<int>(static_cast<uint32_t>(valid_rows * ld * kElementBytes)), 0x00020000);
    auto fill_tile = [&](auto full) __attribute__((always_inline)) {
        u32x4 raw[kPieces];
#pragma unroll
        for (int i = 0; i < kPieces; ++i) {
            const int pid = tid + kThreads * i, n1 = pid / PPS, piece = pid % PPS;
            if (kTotal % kThreads != 0 && pid >= kTotal) break;
            const size_t row = ORDER::template row<N>(N2 * n1 + b);
            if constexpr (decltype(full)::value) {
                const size_t at = (row * ld + f0 + static_cast<size_t>(piece) * PF) * kElementBytes;
                raw[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(held, row < valid_rows ? static_cast<uint32_t>(at) : kBeyondZext, 0, 0));
            } else {
                raw[i] = u32x4{0u, 0u, 0u, 0u};
                if (row < valid_rows) raw[i] = load_piece<DT, false>(x, row, ld, f0, piece, features);
            }
        }
        uint32_t flip[kPieces];                                        // all ones: the piece's row is negated (kSigned alone)
        if constexpr (ROWS::kSigned) {
            uint32_t *flips = reinterpret_cast<uint32_t *>(lds_raw);   // [N1], where the tile will be
            sketch::Key key = rows.value;
            if (rows.device != nullptr) key = *rows.device;            // (one scalar load)
            for (int m = tid; m < N1; m += kThreads) {
                const size_t row = ORDER::template row<N>(N2 * m + b);
                flips[m] = row < valid_rows && row_flipped(key, row) ? 0xffffffffu : 0u;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < kPieces; ++i) {
                const int pid = tid + kThreads * i;
                if (kTotal % kThreads != 0 && pid >= kTotal) break;
                flip[i] = flips[pid / PPS];
            }
            __syncthreads();                                           // (the tables and the tile take this LDS over)
        }
        for (int m = tid; m < N1; m += kThreads) tw[m] = unit(m, N1);
        for (int m = tid; m < kFine; m += kThreads) fine[m] = unit(m, N);
        for (int m = tid; m < kCoarse; m += kThreads) coarse[m] = unit(m * kFine, N);
#pragma unroll
        for (int i = 0; i < kPieces; ++i) {
            const int pid = tid + kThreads * i, n1 = pid / PPS, piece = pid % PPS;
            if (kTotal % kThreads != 0 && pid >= kTotal) break;
            float v[PF];
            if constexpr (ROWS::kSigned) raw[i] ^= sign_bits<DT, decltype(full)::value>(f0 + static_cast<size_t>(piece) * PF, features) & flip[i];
            unpack_piece<DT>(raw[i], v);
            f32x4 *dst = reinterpret_cast<f32x4 *>(tile + n1 * C + piece * (PF / 2));
#pragma unroll
            for (int e = 0; e < PF / 4; ++e) dst[e] = f32x4{v[4 * e], v[4 * e + 1], v[4 * e + 2], v[4 * e + 3]};
        }
    };
    if (f0 + kFeatures <= features) fill_tile(std::true_type{});       // (workgroup-uniform)
    else fill_tile(std::false_type{});
    __syncthreads();

    fft_tile<N1, kRowsA, kSlots>(tile, tw, c, slot);

    constexpr int kUnitsTotal = N1 * (C / 2), kUnits = (kUnitsTotal + kThreads - 1) / kThreads;
#pragma unroll
    for (int i = 0; i < kUnits; ++i) {
        const int uid = tid + kThreads * i, c2 = uid % (C / 2), p = uid / (C / 2);
        if (kUnitsTotal % kThreads != 0 && uid >= kUnitsTotal) break;
        const int k1 = pos_to_freq<N1>(p), e = b * k1;
        const f32x2 w = table_unit(fine, coarse, e, kCoarse > 1);
        const f32x4 z = *reinterpret_cast<const f32x4 *>(tile + p * C + 2 * c2);
        const f32x2 a = cmul(f32x2{z[0], z[1]}, w), bb = cmul(f32x2{z[2], z[3]}, w);
        f32x4 *dst = reinterpret_cast<f32x4 *>(inter + (((2 * t + c2 / (CB / 2)) * N1 + k1) * N2 + b) * CB + 2 * (c2 % (CB / 2)));
        *dst = f32x4{a.x, a.y, bb.x, bb.y};
    }
}

// ---- pass B -----------------------------------------------------------------------------------------------------------------
// The epilogue EPI is what pass B does with Z[k] and Z[N - k] of a sampled k: kTables4N (it wants the tables of W_4N in LDS behind the
// tile), factor (host: what the kernel is given as `scale`), prepare (what a thread computes once) and write (the values of one sampled
// row that a lane holds, and their stores).
// The cosine rows (fewbit_dct.hip, steps 1 and 2): out[j][:] in ODT.  LIBRARY is a tag and nothing else: the DCT's pass B is compiled
// into both shared libraries, and the tag gives each its own kernel symbols.
struct CoreLibrary;                         // libfewbit_hip.so
struct CompanionLibrary;                    // libfewbit_hipx.so
template <typename LIBRARY> struct CosineRows {
    static constexpr bool kTables4N = true;                            // e^{-i pi k / 2N} = W_4N^k
    static float factor(double scale, size_t) { return static_cast<float>(scale); }
    float base;
    template <int N> __device__ __forceinline__ void prepare(float scale, size_t, size_t) {
        base = scale * __builtin_sqrtf(0.5f / static_cast<float>(N));                      // ortho: sqrt(1 / 2N) (k > 0), sqrt(1 / 4N) (k = 0)
    }
    template <int ODT, int E, int N>
    __device__ __forceinline__ void write(const f32x2 (&zk)[E], const f32x2 (&zm)[E], int km, const f32x2 *fine, const f32x2 *coarse, void *out, size_t j,
                                          size_t features, size_t fa) const {
        const f32x2 w = table_unit(fine, coarse, km, coarse_entries(N) > 1);            // e^{-i pi k / 2N}
        const float f = (km == 0 ? kR2 : 1.0f) * 2.0f * base;
        float y[2 * E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            f32x2 m = zm[e];
            m.y = -m.y;                                                 // conj Z[N - k]
            const f32x2 va = (zk[e] + m) * 0.5f, d = (zk[e] - m) * 0.5f, vb = mul_mi(d);
            y[2 * e] = (w.x * va.x - w.y * va.y) * f;                   // Re(w V)
            y[2 * e + 1] = (w.x * vb.x - w.y * vb.y) * f;
        }
        store_values<ODT, E>(out, j * features + fa, y, fa, features);
    }
};
// The Fourier planes (fewbit_dft.hip): out: [2][proj][features] in ODT (real plane, imaginary plane); no e^{-i pi k / 2N} twiddle, so no
// W_4N tables, and no sqrt(2) at k = 0.
struct FourierPlanes {
    static constexpr bool kTables4N = false;
    static float factor(double scale, size_t rows) { return static_cast<float>(scale / std::sqrt(static_cast<double>(rows))); }
    float half;
    size_t plane;
    template <int N> __device__ __forceinline__ void prepare(float factor, size_t proj, size_t features) {
        half = 0.5f * factor;
        plane = proj * features;
    }
    template <int ODT, int E, int N>
    __device__ __forceinline__ void write(const f32x2 (&zk)[E], const f32x2 (&zm)[E], int, const f32x2 *, const f32x2 *, void *out, size_t j, size_t features,
                                          size_t fa) const {
        // a = Z[k], b = Z[N - k]:  X_2c = (a + conj b) / 2,  X_2c+1 = (a - conj b) / 2i = ((a.y + b.y) + i (b.x - a.x)) / 2
        float re[2 * E], im[2 * E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const f32x2 a = zk[e], b = zm[e];
            re[2 * e] = (a.x + b.x) * half;
            im[2 * e] = (a.y - b.y) * half;
            re[2 * e + 1] = (a.y + b.y) * half;
            im[2 * e + 1] = (b.x - a.x) * half;
        }
        const size_t at = j * features + fa;
        store_values<ODT, E>(out, at, re, fa, features);
        store_values<ODT, E>(out, plane + at, im, fa, features);
    }
};

// grid (N1 / 2 + 1, half tiles of 16 complex columns): residues k1 = u and (N1 - u) % N1.  The LDS tile is [N2][2][16]: the two
// residue rows sit side by side, so that a half-wave still touches 256 contiguous bytes per position and one butterfly serves
// both rows -- to the transform it is one row of 32 columns.  scale: EPI::factor of the call.
template <typename EPI, int ODT, int N1, int N2>
__global__ __launch_bounds__(kThreadsB, (N2 > 128 ? 2 : 4)) void pass_b_kernel(const f32x2 *__restrict__ inter, const int *__restrict__ offsets, const Sample *__restrict__ sorted,
                                                              size_t proj, size_t features, float scale, void *__restrict__ out) {
    constexpr int N = N1 * N2, kCoarse = coarse_entries(N), kThreads = kThreadsB, kSlots = kThreads / C;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    f32x2 *tile = reinterpret_cast<f32x2 *>(lds_raw);                 // [N2][2][CB]
    f32x2 *tw = tile + N2 * 2 * CB;                                   // W_N2^m
    f32x2 *fine = tw + N2, *coarse = fine + kFine;                    // kTables4N: W_4N^m (m < 128), W_4N^{128 m}
    const int tid = threadIdx.x;
    const int u = blockIdx.x, k1a = u, k1b = (N1 - u) % N1;
    const size_t t = blockIdx.y, f0 = t * (2 * CB);
    // four lanes write one sampled row, four complex columns each: 64 rows at a time -- all of a typical workgroup's in one step (with 16
    // lanes per row the four dependent steps of sample -> tile -> table -> store cost 1.5 us of a 18.8 us launch, profiles/r06_dct_serve_lanes.txt)
    constexpr int kLanes = kServeLanes, E = CB / kLanes, kSGroups = kThreads / kLanes;       // lanes per sample, complex columns per lane
    const int lane = tid % kLanes, sgroup = tid / kLanes;

    // this workgroup's samples (pass A's workgroup (0, 0) sorted them): the first two of every group of lanes are requested FIRST (vmcnt
    // counts in order: looking at them after the transform does not wait for anything), unconditionally (a clamped index: hipcc gives a
    // load under a lane-divergent guard its own wait)
    const int begin = offsets[u], count = offsets[u + 1] - begin;      // (scalar loads)
    constexpr int kPre = 2;
    Sample pre[kPre];
#pragma unroll
    for (int i = 0; i < kPre; ++i) {
        const size_t e = static_cast<size_t>(begin) + sgroup + i * kSGroups;
        pre[i] = sorted[e < proj ? e : proj - 1];
    }
    constexpr int kPerRow = N2 * (CB / 2), kTotal = 2 * kPerRow, kPieces = (kTotal + kThreads - 1) / kThreads;     // 16-byte pieces (two complex)
    f32x4 v[kPieces];
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
        const int pid = tid + kThreads * i, r = pid / kPerRow, rest = pid % kPerRow;
        if (kTotal % kThreads != 0 && pid >= kTotal) break;
        const f32x2 *src = inter + (t * N1 + (r == 0 ? k1a : k1b)) * static_cast<size_t>(N2) * CB;
        v[i] = reinterpret_cast<const f32x4 *>(src)[rest];
    }
    for (int m = tid; m < N2; m += kThreads) tw[m] = unit(m, N2);
    if constexpr (EPI::kTables4N) {
        for (int m = tid; m < kFine; m += kThreads) fine[m] = unit(m, 4 * N);
        for (int m = tid; m < kCoarse; m += kThreads) coarse[m] = unit(m * kFine, 4 * N);
    }
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
        const int pid = tid + kThreads * i, r = pid / kPerRow, rest = pid % kPerRow, n2 = rest / (CB / 2), c2 = rest % (CB / 2);
        if (kTotal % kThreads != 0 && pid >= kTotal) break;
        *reinterpret_cast<f32x4 *>(tile + (n2 * 2 + r) * CB + 2 * c2) = v[i];
    }
    __syncthreads();
    fft_tile<N2, 1, kSlots>(tile, tw, tid % C, tid / C);               // (ends with a barrier)

    // ---- the sampled rows of this workgroup's two residue classes: one per group of kServeLanes lanes at a time, lanes along the columns
    EPI epilogue;
    epilogue.template prepare<N>(scale, proj, features);
    auto write_row = [&](int km, size_t j) __attribute__((always_inline)) {
        const int k1 = km % N1, k2 = km / N1;
        const int r = k1 == k1a ? 0 : 1;
        const int k2m = k1 == 0 ? (N2 - k2) % N2 : N2 - 1 - k2;         // N - k = (N1 - k1) + N1 k2m
        const f32x2 *pk = tile + (freq_to_pos<N2>(k2) * 2 + r) * CB + E * lane;
        const f32x2 *pm = tile + (freq_to_pos<N2>(k2m) * 2 + (1 - r)) * CB + E * lane;
        f32x2 zk[E], zm[E];
        if constexpr (E >= 2) {
#pragma unroll
            for (int e = 0; e < E; e += 2) {
                const f32x4 a4 = *reinterpret_cast<const f32x4 *>(pk + e), b4 = *reinterpret_cast<const f32x4 *>(pm + e);
                zk[e] = f32x2{a4[0], a4[1]}; zk[e + 1] = f32x2{a4[2], a4[3]};
                zm[e] = f32x2{b4[0], b4[1]}; zm[e + 1] = f32x2{b4[2], b4[3]};
            }
        } else {
            zk[0] = pk[0]; zm[0] = pm[0];
        }
        epilogue.template write<ODT, E, N>(zk, zm, km, fine, coarse, out, j, features, f0 + 2 * E * lane);
    };
#pragma unroll
    for (int i = 0; i < kPre; ++i)
        if (sgroup + i * kSGroups < count) write_row(pre[i].k, static_cast<size_t>(pre[i].j));
    // (more than 128 samples in these two classes: p beyond ~8000, or a skewed idx)
    for (int e = sgroup + kPre * kSGroups; e < count; e += kSGroups) {
        const Sample smp = sorted[static_cast<size_t>(begin) + e];
        write_row(smp.k, static_cast<size_t>(smp.j));
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
struct Split { int n1, n2; };
// rows = N1 x N2.  2^8 .. 2^18: 16 <= N2 <= N1 <= 512, both powers of two (2^17 = 512 x 256 and 2^18 = 512 x 512: 128 KiB tiles, one
// workgroup per CU).  3 x 2^8 .. 3 x 2^14 (768 .. 49152), 5 x 2^8 .. 5 x 2^13 (1280 .. 40960), 7 x 2^9 .. 7 x 2^13 (3584 .. 57344),
// 9 x 2^8 .. 9 x 2^12 (2304 .. 36864) and 15 x 2^8 .. 15 x 2^11 (3840 .. 30720): the odd factor goes to the second pass, N2 = 48 / 96 /
// 192, 80 / 160, 112 / 224, 144 / 288 or 240 (N1 stays a power of two: residues and digit maps of pass A, the k % N1 of pass B).  Pass
// B's tile is 256 N2 bytes + tables: at most 78 KiB (N2 = 288), two workgroups in the 160 KiB of a CU
struct RowFamily { int odd, low, high, n1[7]; };       // rows = odd x 2^bits, low <= bits <= high; n1[bits - low]
constexpr int kLowBits = 8, kHighBits = 18;            // rows = 2^bits: 256 .. 262144
// N1 grows with the rows up to 128 (four pass-A workgroups per CU) before N2 doubles, and reaches 256 last:
//  3 x 2^bits, bits = 8 .. 14:  16 x 48, 32 x 48, 32 x 96, 64 x 96, 128 x 96, 128 x 192, 256 x 192
//  5 x 2^bits, bits = 8 .. 13:  16 x 80, 32 x 80, 64 x 80, 64 x 160, 128 x 160, 256 x 160
//  7 x 2^bits, bits = 9 .. 13:  32 x 112 (3584), 64 x 112 (7168), 128 x 112 (14336), 128 x 224 (28672), 256 x 224 (57344)
//  9 x 2^bits, bits = 8 .. 12:  16 x 144 (2304), 32 x 144 (4608), 64 x 144 (9216), 128 x 144 (18432), 128 x 288 (36864)
// 15 x 2^bits, bits = 8 .. 11:  16 x 240 (3840), 32 x 240 (7680), 64 x 240 (15360), 128 x 240 (30720)
// (15 and 9 before 5 and 3: a multiple of 15 is one of 3 and of 5)
constexpr int kRowFamilyCount = 5;
inline const RowFamily *row_families() {
    static const RowFamily families[kRowFamilyCount] = {{15, 8, 11, {16, 32, 64, 128}},
                                                        {9, 8, 12, {16, 32, 64, 128, 128}},
                                                        {7, 9, 13, {32, 64, 128, 128, 256}},
                                                        {5, 8, 13, {16, 32, 64, 64, 128, 256}},
                                                        {3, 8, 14, {16, 32, 32, 64, 128, 128, 256}}};
    return families;
}
inline bool split_rows(size_t rows, Split &s) {
    if (rows < (static_cast<size_t>(1) << kLowBits) || rows > (static_cast<size_t>(1) << kHighBits)) return false;
    const RowFamily *families = row_families();
    const RowFamily *family = nullptr;
    for (int i = 0; i < kRowFamilyCount; ++i)
        if (family == nullptr && rows % static_cast<size_t>(families[i].odd) == 0) family = &families[i];
    const size_t two = family != nullptr ? rows / static_cast<size_t>(family->odd) : rows;
    if (!power_of_two(two)) return false;
    int bits = 0;
    while ((static_cast<size_t>(1) << bits) < two) ++bits;
    if (family == nullptr) {
        s.n1 = 1 << ((bits + 1) / 2);
        s.n2 = 1 << (bits / 2);
        return true;
    }
    if (bits < family->low || bits > family->high) return false;
    s.n1 = family->n1[bits - family->low];
    s.n2 = static_cast<int>(rows / static_cast<size_t>(s.n1));
    return true;
}
// the smallest row count split_rows takes that is >= rows, from the same table: of 2^bits and of every family the first member that
// reaches `rows`, and of those the least; 0 for rows = 0 and beyond the largest (what a zero-extended call runs at)
inline size_t rows_ceil(size_t rows) {
    if (rows == 0 || rows > (static_cast<size_t>(1) << kHighBits)) return 0;
    size_t best = 0;
    auto offer = [&](size_t odd, int low, int high) {
        for (int bits = low; bits <= high; ++bits) {
            const size_t n = odd << bits;
            if (n < rows) continue;
            if (best == 0 || n < best) best = n;
            return;
        }
    };
    offer(1, kLowBits, kHighBits);
    const RowFamily *families = row_families();
    for (int i = 0; i < kRowFamilyCount; ++i) offer(static_cast<size_t>(families[i].odd), families[i].low, families[i].high);
    return best;
}
// the (N1, N2) split_rows returns: the cases of the launches and of the LDS opt-in
#define FB_FFT4_SPLITS(X)                                                                                                     \
    X(16, 16) X(32, 16) X(32, 32) X(64, 32) X(64, 64) X(128, 64) X(128, 128) X(256, 128) X(256, 256) X(512, 256) X(512, 512) \
    X(16, 48) X(32, 48) X(32, 96) X(64, 96) X(128, 96) X(128, 192) X(256, 192)                                                \
    X(16, 80) X(32, 80) X(64, 80) X(64, 160) X(128, 160) X(256, 160)                                                          \
    X(32, 112) X(64, 112) X(128, 112) X(128, 224) X(256, 224)                                                                 \
    X(16, 144) X(32, 144) X(64, 144) X(128, 144) X(128, 288)                                                                  \
    X(16, 240) X(32, 240) X(64, 240) X(128, 240)
// the row counts split_rows takes, as every refusal names them
constexpr char kRowFamilies[] = "2^k (256 .. 262144), 3 x 2^k (768 .. 49152), 5 x 2^k (1280 .. 40960), 7 x 2^k (3584 .. 57344), 9 x 2^k (2304 .. 36864), "
                              "15 x 2^k (3840 .. 30720)";

inline size_t tiles_of(size_t features) { return (features + kFeatures - 1) / kFeatures; }
inline size_t inter_bytes(size_t rows, size_t features) { return tiles_of(features) * rows * C * sizeof(f32x2); }
// workspace: [the intermediate | offsets of the sorted samples (2 KiB) | the sorted samples, 8 bytes each]
inline size_t workspace_bytes_of(size_t rows, size_t features, size_t proj) { return inter_bytes(rows, features) + kOffsetsBytes + ((proj * sizeof(Sample) + 15) & ~static_cast<size_t>(15)); }

template <int L> constexpr size_t lds_bytes_a(int n) { return (kRowsA * L * C + L + kFine + coarse_entries(n)) * sizeof(f32x2); }
template <typename EPI, int L> constexpr size_t lds_bytes_b(int n) { return (2 * L * CB + L + (EPI::kTables4N ? kFine + coarse_entries(n) : 0)) * sizeof(f32x2); }

using unit::known_dtype;
inline RowsOfSeed rows_of_seed(uint64_t seed, const uint64_t *device) {
    return RowsOfSeed{sketch::key_of(seed), reinterpret_cast<const sketch::Key *>(device)};
}

// ---- the host side of the kernel pairs --------------------------------------------------------------------------------------
// PAIR (fewbit_dct.hip: Dct, DctZext; fewbit_dft.hip: Dft, DftZext; fewbit_signed.hip: DctSigned, DftSigned) names what differs between
// them: Order (the rows of pass A: RowsMakhoul / RowsInOrder), Epilogue (of pass B: CosineRows / FourierPlanes), kZext (its pass A is a
// pass_a_zext_kernel and takes valid_rows), PassB (the pair whose pass B it runs -- a plain pair: itself -- and with it whose LDS opt-in
// covers those kernels), kSeededLast (below), the prefix of its messages (kName), its workspace query (kWorkspace) and its error reporter
// (fail: each library keeps its own last error); a pair with the signs of the seed also Unsigned, the zero-extended pair it extends.
// The kernels, pass B's LDS and the factor pass B applies follow from those, here:
template <typename PAIR, int DT, int N1, int N2, typename ROWS> constexpr auto pass_a_of() {
    if constexpr (PAIR::kZext) return &pass_a_zext_kernel<typename PAIR::Order, DT, N1, N2, ROWS>;
    else return &pass_a_kernel<typename PAIR::Order, DT, N1, N2, ROWS>;
}
template <typename PAIR, int ODT, int N1, int N2> constexpr auto pass_b_of() { return &pass_b_kernel<typename PAIR::Epilogue, ODT, N1, N2>; }
template <typename PAIR, int N1, int N2> constexpr size_t lds_b_of() { return lds_bytes_b<typename PAIR::Epilogue, N2>(N1 * N2); }

template <typename PAIR> int refuse_rows(const char *what, size_t rows) {
    return PAIR::fail(FEWBIT_ERR_UNSUPPORTED, "%s: rows = %zu is none of %s", what, rows, kRowFamilies);
}

template <typename PAIR, typename K> int reserve_lds(K kern, size_t lds) {
    if (lds <= 65536) return FEWBIT_OK;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) != hipSuccess) {
        (void)hipGetLastError();
        return PAIR::fail(FEWBIT_ERR_LAUNCH, "%s: cannot reserve %zu bytes of LDS", PAIR::kName, lds);
    }
    return FEWBIT_OK;
}

// The LDS opt-ins below run once per device, at the first call that needs them -- not per instantiation at its own first launch: after
// one eager call of a dtype, a hipGraph capture of any other row count of that dtype makes no attribute call.  `done` is the opt-in's
// own set of devices; `reserve` is run until it has succeeded once on the current one.
template <typename F> int once_per_device(std::atomic<unsigned long long> &done, F &&reserve) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_relaxed) & bit) return FEWBIT_OK;
    const int rc = reserve();
    if (rc == FEWBIT_OK) done.fetch_or(bit, std::memory_order_relaxed);
    return rc;
}
#define FB_FFT4_RESERVE_A(ROWS, A, B) if (rc == FEWBIT_OK) rc = reserve_lds<PAIR>(pass_a_of<PAIR, DT, A, B, ROWS>(), lds_bytes_a<A>(A * B));
#define FB_FFT4_RESERVE_B(A, B) if (rc == FEWBIT_OK) rc = reserve_lds<PAIR>(pass_b_of<PAIR, DT, A, B>(), lds_b_of<PAIR, A, B>());

// the LDS opt-in of every pass B of PAIR that writes DT alone: a pair whose pass A is zero-extended only (the DCT's in the companion library)
template <typename PAIR, int DT> int opt_in_pass_b() {
    static std::atomic<unsigned long long> done{0};
    return once_per_device(done, [] {
        int rc = FEWBIT_OK;
        FB_FFT4_SPLITS(FB_FFT4_RESERVE_B)
        return rc;
    });
}

// The LDS opt-in of EVERY kernel of dtype DT whose tile exceeds 64 KiB (pass A reading DT, for both kinds of rows, and pass B writing
// DT).  Pass B of a zero-extended pair is another pair's, reserved by that pair's opt-in, or its own, by opt_in_pass_b.
template <typename PAIR, int DT> int opt_in_dtype() {
    static std::atomic<unsigned long long> done{0};
    return once_per_device(done, [] {
        int rc = FEWBIT_OK;
        if constexpr (PAIR::kZext) {
            if constexpr (std::is_same_v<typename PAIR::PassB, PAIR>) rc = opt_in_pass_b<PAIR, DT>();
            else rc = opt_in_dtype<typename PAIR::PassB, DT>();
        }
        // (the order in which a unit first names its kernels is their order in the device module, and the code generated for the last
        // split depends on it: each pair names them in the order of its former host code -- the DCT's seeded pass A after all others)
#define FB_FFT4_OPT_IN(A, B)                                                  \
    FB_FFT4_RESERVE_A(RowsInMemory, A, B)                                     \
    if constexpr (!PAIR::kSeededLast) FB_FFT4_RESERVE_A(RowsOfSeed, A, B)     \
    if constexpr (!PAIR::kZext) FB_FFT4_RESERVE_B(A, B)
#define FB_FFT4_OPT_IN_SEEDED(A, B) FB_FFT4_RESERVE_A(RowsOfSeed, A, B)
        FB_FFT4_SPLITS(FB_FFT4_OPT_IN)
        if constexpr (PAIR::kSeededLast) { FB_FFT4_SPLITS(FB_FFT4_OPT_IN_SEEDED) }
#undef FB_FFT4_OPT_IN
#undef FB_FFT4_OPT_IN_SEEDED
        return rc;
    });
}

// the LDS opt-in of a pair whose pass A takes the signs of the seed (fewbit_signed.hip): that of the zero-extended pair it extends, whose
// pass B it runs, and its own pass A reading DT -- at the first signed call of DT
template <typename PAIR, int DT> int opt_in_signed() {
    static std::atomic<unsigned long long> done{0};
    return once_per_device(done, [] {
        int rc = opt_in_dtype<typename PAIR::Unsigned, DT>();
#define FB_FFT4_OPT_IN_SIGNED(A, B) FB_FFT4_RESERVE_A(SignedRowsOfSeed, A, B)
        FB_FFT4_SPLITS(FB_FFT4_OPT_IN_SIGNED)
#undef FB_FFT4_OPT_IN_SIGNED
        return rc;
    });
}
#undef FB_FFT4_RESERVE_A
#undef FB_FFT4_RESERVE_B

// (valid_rows: the rows of m in memory, for a zero-extended pair; a plain pair's kernels do not take it)
template <typename PAIR, int DT, typename ROWS>
int launch_a(Split sp, const void *m, size_t valid_rows, size_t features, size_t ld, ROWS idx, size_t proj, f32x2 *inter, int *offsets, Sample *sorted, hipStream_t s) {
    const unsigned tiles = static_cast<unsigned>(tiles_of(features));
#define FB_FFT4_CASE_A(A, B)                                                                                                   \
    if (sp.n1 == A && sp.n2 == B) {                                                                                            \
        static_assert(lds_bytes_a<A>(A * B) >= 2 * (A / 2 + 2) * sizeof(int) && (A / 2 + 2) * sizeof(int) <= kOffsetsBytes,    \
                      "the sort's counters fit pass A's LDS and the offsets their slot");                                      \
        constexpr auto kern = pass_a_of<PAIR, DT, A, B, ROWS>();                                                               \
        auto launch = [&](auto... held) {                                                                                      \
            hipLaunchKernelGGL(kern, dim3(B, tiles), dim3(kThreadsA), lds_bytes_a<A>(A * B), s, m, held..., features, ld, inter, idx, proj, offsets, sorted); \
        };                                                                                                                     \
        if constexpr (PAIR::kZext) launch(valid_rows);                                                                         \
        else launch();                                                                                                         \
        return FEWBIT_OK;                                                                                                      \
    }
    FB_FFT4_SPLITS(FB_FFT4_CASE_A)
#undef FB_FFT4_CASE_A
    return PAIR::fail(FEWBIT_ERR_UNSUPPORTED, "%s: no kernel for %d x %d rows", PAIR::kName, sp.n1, sp.n2);
}

template <typename PAIR, int ODT>
int launch_b(Split sp, const f32x2 *inter, const int *offsets, const Sample *sorted, size_t proj, size_t features, float factor, void *out, hipStream_t s) {
    const unsigned half_tiles = static_cast<unsigned>((features + 2 * CB - 1) / (2 * CB));
#define FB_FFT4_CASE_B(A, B)                                                                                                   \
    if (sp.n1 == A && sp.n2 == B) {                                                                                            \
        constexpr auto kern = pass_b_of<PAIR, ODT, A, B>();                                                                    \
        hipLaunchKernelGGL(kern, dim3(A / 2 + 1, half_tiles), dim3(kThreadsB), (lds_b_of<PAIR, A, B>()), s, inter, offsets, sorted, proj, features, factor, out); \
        return FEWBIT_OK;                                                                                                      \
    }
    FB_FFT4_SPLITS(FB_FFT4_CASE_B)
#undef FB_FFT4_CASE_B
    return PAIR::fail(FEWBIT_ERR_UNSUPPORTED, "%s: no kernel for %d x %d rows", PAIR::kName, sp.n1, sp.n2);
}

// the host functions of dtype DT: a pair is compiled as three translation units, one per dtype, each instantiating its own (KEYWORD
// empty); the unit with the C entry points declares the other two (KEYWORD extern).  Used in namespace fewbit_hip or fewbit_hip::dct.
#define FB_FFT4_UNIT_A(KEYWORD, PAIR, DT)                                                                                      \
    KEYWORD template int dct::opt_in_dtype<PAIR, DT>();                                                                        \
    KEYWORD template int dct::launch_a<PAIR, DT, dct::RowsInMemory>(dct::Split, const void *, size_t, size_t, size_t, dct::RowsInMemory, size_t, dct::f32x2 *, int *, dct::Sample *, hipStream_t); \
    KEYWORD template int dct::launch_a<PAIR, DT, dct::RowsOfSeed>(dct::Split, const void *, size_t, size_t, size_t, dct::RowsOfSeed, size_t, dct::f32x2 *, int *, dct::Sample *, hipStream_t);
#define FB_FFT4_UNIT_B(KEYWORD, PAIR, DT) \
    KEYWORD template int dct::launch_b<PAIR, DT>(dct::Split, const dct::f32x2 *, const int *, const dct::Sample *, size_t, size_t, float, void *, hipStream_t);
#define FB_FFT4_UNIT(KEYWORD, PAIR, DT) FB_FFT4_UNIT_A(KEYWORD, PAIR, DT) FB_FFT4_UNIT_B(KEYWORD, PAIR, DT)
// (a pair with the signs of the seed has a unit of that pass A alone)
#define FB_FFT4_UNIT_SIGNED(KEYWORD, PAIR, DT)                                                                                 \
    KEYWORD template int dct::opt_in_signed<PAIR, DT>();                                                                       \
    KEYWORD template int dct::launch_a<PAIR, DT, dct::SignedRowsOfSeed>(dct::Split, const void *, size_t, size_t, size_t, dct::SignedRowsOfSeed, size_t, dct::f32x2 *, int *, dct::Sample *, hipStream_t);
// (a zero-extended pair whose pass B is another pair's has a unit of pass A alone: FB_FFT4_UNIT_A)

// calls f(std::integral_constant<int, DT>) for the run-time dtype (one of known_dtype)
template <typename F> int with_dtype(int dtype, F &&f) {
    switch (dtype) {
    case FEWBIT_F32: return f(std::integral_constant<int, FEWBIT_F32>{});
    case FEWBIT_F16: return f(std::integral_constant<int, FEWBIT_F16>{});
    default: return f(std::integral_constant<int, FEWBIT_BF16>{});
    }
}

// One call of a pair: the argument checks, the LDS opt-in of the dtypes involved, the workspace carved into [inter | offsets | sorted],
// pass A reading `dtype`, pass B writing `out_dtype` (the DCT's is its dtype), and the launch error.  valid_rows: the rows m holds, of a
// zero-extended pair (a plain pair: rows).
template <typename PAIR, typename ROWS>
int run(int dtype, int out_dtype, const void *m, size_t rows, size_t valid_rows, size_t features, size_t ld, ROWS idx, size_t proj, double scale, void *out,
        void *workspace, size_t workspace_bytes, void *stream) {
    const char *name = PAIR::kName;
    if (!known_dtype(dtype)) return PAIR::fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: unknown dtype %d", name, dtype);
    if (out_dtype != FEWBIT_F32 && out_dtype != dtype) return PAIR::fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: out_dtype %d is neither F32 nor the dtype of m", name, out_dtype);
    if (proj == 0 || features == 0) return FEWBIT_OK;
    if constexpr (ROWS::kSeeded)
        if ((reinterpret_cast<uintptr_t>(idx.device) & 7) != 0) return PAIR::fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: the seed word in device memory must be 8-byte aligned", name);
    Split sp;
    if (!split_rows(rows, sp)) return refuse_rows<PAIR>(name, rows);
    if (valid_rows == 0 || valid_rows > rows) return PAIR::fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: valid_rows = %zu is not in 1 .. rows = %zu", name, valid_rows, rows);
    if constexpr (PAIR::kZext)
        if (!zext_span_ok(valid_rows, ld, dtype)) return PAIR::fail(FEWBIT_ERR_UNSUPPORTED, "%s: valid_rows x ld = %zu x %zu elements span 4 GiB or more", name, valid_rows, ld);
    bool null = m == nullptr || out == nullptr;
    if constexpr (!ROWS::kSeeded) null = null || idx.idx == nullptr;
    if (null) return PAIR::fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: null pointer", name);
    if (ld < features) return PAIR::fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: leading dimension %zu < features %zu", name, ld, features);
    const size_t need = workspace_bytes_of(rows, features, proj);
    if (workspace == nullptr || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0)
        return PAIR::fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: a 16-byte aligned workspace of %zu bytes is needed (%s), got %zu", name, need, PAIR::kWorkspace, workspace_bytes);
    if (tiles_of(features) > 32767) return PAIR::fail(FEWBIT_ERR_UNSUPPORTED, "%s: more than 32767 column tiles", name);
    if (proj > 0x7fffffffull) return PAIR::fail(FEWBIT_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 samples", name);
    auto opt_in = [](auto dt) {
        if constexpr (ROWS::kSigned) return opt_in_signed<PAIR, decltype(dt)::value>();
        else return opt_in_dtype<PAIR, decltype(dt)::value>();
    };
    if (const int rc = with_dtype(dtype, opt_in)) return rc;
    if (out_dtype != dtype)
        if (const int rc = with_dtype(out_dtype, opt_in)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    f32x2 *inter = static_cast<f32x2 *>(workspace);
    int *offsets = reinterpret_cast<int *>(static_cast<uint8_t *>(workspace) + inter_bytes(rows, features));
    Sample *sorted = reinterpret_cast<Sample *>(reinterpret_cast<uint8_t *>(offsets) + kOffsetsBytes);
    if (const int rc = with_dtype(dtype, [&](auto dt) { return launch_a<PAIR, decltype(dt)::value, ROWS>(sp, m, valid_rows, features, ld, idx, proj, inter, offsets, sorted, s); }))
        return rc;
    const float factor = PAIR::Epilogue::factor(scale, rows);
    if (const int rc = with_dtype(out_dtype, [&](auto dt) { return launch_b<typename PAIR::PassB, decltype(dt)::value>(sp, inter, offsets, sorted, proj, features, factor, out, s); }))
        return rc;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return PAIR::fail(FEWBIT_ERR_LAUNCH, "%s: %s", name, hipGetErrorString(e));
    return FEWBIT_OK;
}

}  // namespace dct
}  // namespace fewbit_hip
