// fewbit_mxdef.h -- the definition of "the row blocks of a seed" (include/fewbit_hipx.h): a rows x width matrix kept as OCP-MX cells that run DOWN
// its columns, so that a cell is the operand fragment of one lane of v_mfma_scale_f32_32x32x64_f8f6f4 when the rows are the K dimension (the weight
// gradient G^T X).  The ONE text that fewbit_mx.hip evaluates on the host and on the device, one element at a time and in integer arithmetic only:
// no fp32 operation takes part in a code, so denormal modes, contraction and the rounding of a division cannot make host and device differ.
//
//   cell (b, j)   rows 32 b .. 32 b + 31 of column j; rows >= `rows` count as +0.  One E8M0 scale byte and 32 element codes.
//   formats       fp4 = E2M1 (largest value 6), fp6 = E2M3 (7.5), fp8 = E4M3 (448; S.1111.111 is its NaN).  Named by their bits: 4, 6, 8.
//   scale         e = the smallest integer with amax * 2^-e <= the largest value, clamped to -127 .. 127; the byte is e + 127.  Read from the
//                 exponent and the significand of amax (a denormal amax is normalised first): e = exponent(amax) - exponent(largest), plus one
//                 where the significand of amax is above that of the largest value.  NOT the OCP recipe floor(log2 amax) - emax, which clips
//                 the top of each binade and so biases the estimate.  amax = 0: e = -127, every code +0.
//   poison        a cell that holds a NaN or an infinity stores scale byte 0xFF (E8M0's NaN) and decodes to NaN as a whole; its codes are 0 at
//                 fp4 and fp6 and 0x7F (the format's own NaN) at fp8.
//   code          t = |v| * 2^-e, exact as a real number (never formed in fp32); lo <= t <= hi the neighbouring magnitudes of the format; the
//                 code is hi's where (t - lo) / (hi - lo) + U >= 1, else lo's, with the sign bit of v.  U = u / 65536, u the 16 Philox bits
//                 of the element (uniform_of's bits).  With f = (t - lo) / (hi - lo): f + U >= 1 <=> floor(65536 f) + u >= 65536 (u is an
//                 integer), so the fraction is cut to 16 bits without changing any decision: E[decode] = v to the 2^-16 granularity of U.
//   tiny cells    e is clamped at -127, so t never needs 2^-e beyond 2^127; an element far below its cell's amax (|v| 2^-e below 2^-25 of the
//                 smallest magnitude) has floor(65536 f) = 0 and code +-0 whatever the denormal mode would have done to the product: there is
//                 no fp32 product.  A denormal element is normalised in integers like a denormal amax.
//   decode        magnitude * 2^e, exact in fp32 (denormal results included); beyond FLT_MAX (a cell whose amax is within a step of it) it is inf.
//   Philox        one call per eight consecutive rows of one column: counter words (lo, hi of q, 0, domain), q = 4 (b * width + j) + octet,
//                 octet = (row % 32) / 8; element row % 8 of the call (mask_bits).  domain 9: a kept input, 10: a gradient.
//   layout        scales [ceil(rows / 32)][width] bytes; codes from the next multiple of 16: [ceil(rows / 32)][width][cell], a cell 16 / 24 / 32
//                 bytes: element r of the cell at bits [bits r, bits (r + 1)) of the cell taken as one little-endian number (fp4: low nibble
//                 first; fp6: a little-endian bit stream over 6 dwords; fp8: a byte each).  At fp4 and fp6 that is the order of the 32 K values of
//                 one lane of the instruction, a cell is a lane's operand.  At fp8 the hardware differs from that picture (measured with one-hot
//                 cells): a lane holds two runs of 16 K values, K 16 h .. and K 32 + 16 h .., so the product kernel takes 16 bytes from each of
//                 the two cells of a K step (fewbit_mx.hip); the layout here stays row order for every format.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "fewbit_hipx.h"
#include "fewbit_philox.h"
#include "fewbit_quantdef.h"

namespace fewbit_hip {
namespace mx {

using namespace quant;                      // (bits_of_float, float_of_bits, non_finite, narrow, widen, Elem, the predicates and the refusals of fewbit_unit.h)

constexpr int kCellRows = 32, kOctets = kCellRows / kBlock;
constexpr uint32_t kKeptDomain = 9u, kGradDomain = 10u;       // counter word 3 (0 and 2 .. 8 are taken: fewbit_quantdef.h)
constexpr uint32_t kPoisonScale = 0xFFu;
constexpr size_t kMaxWidth = size_t{1} << 23;

// a format by its bits: mantissa bits, the exponent of the smallest normal, the largest value as (24-bit significand, exponent), its code
template <int FMT> struct Format;
template <> struct Format<4> { static constexpr int M = 1, emin = 0, qmax = 2; static constexpr uint32_t sigmax = 0xC00000u, codemax = 0x7u; };
template <> struct Format<6> { static constexpr int M = 3, emin = 0, qmax = 2; static constexpr uint32_t sigmax = 0xF00000u, codemax = 0x1Fu; };
template <> struct Format<8> { static constexpr int M = 3, emin = -6, qmax = 8; static constexpr uint32_t sigmax = 0xE00000u, codemax = 0x7Eu; };

inline bool known_format(int format) { return format == 4 || format == 6 || format == 8; }
__host__ __device__ constexpr size_t cell_bytes(int format) { return 4 * static_cast<size_t>(format); }
inline uint32_t domain_of(int role) { return role == 0 ? kKeptDomain : kGradDomain; }

__host__ __device__ inline size_t blocks_of(size_t rows) { return (rows + kCellRows - 1) / kCellRows; }
__host__ __device__ inline size_t codes_offset(size_t rows, size_t width) { return (blocks_of(rows) * width + 15) / 16 * 16; }
inline size_t bytes_of(size_t rows, size_t width, int format) {
    if (!known_format(format) || rows == 0 || width == 0 || width > kMaxWidth || rows > kMaxCount / width) return 0;
    return codes_offset(rows, width) + blocks_of(rows) * width * cell_bytes(format);
}

// |v| as (24-bit significand with its leading one at bit 23, exponent): |v| = sig * 2^(x - 23); zero: sig = 0
struct Norm { uint32_t sig; int x; };
__host__ __device__ __forceinline__ Norm normalise(uint32_t magnitude_bits) {
    const uint32_t field = magnitude_bits >> 23, frac = magnitude_bits & 0x7fffffu;
    if (field != 0) return Norm{frac | 0x800000u, static_cast<int>(field) - 127};
    if (frac == 0) return Norm{0u, -126};
    const int shift = __builtin_clz(frac) - 8;
    return Norm{frac << shift, -126 - shift};
}

// the scale exponent e of a cell from the bits of its amax (finite)
template <int FMT> __host__ __device__ __forceinline__ int scale_of_amax(uint32_t amax_bits) {
    using F = Format<FMT>;
    const Norm a = normalise(amax_bits);
    if (a.sig == 0) return -127;
    const int e = a.x - F::qmax + (a.sig > F::sigmax ? 1 : 0);
    return e < -127 ? -127 : e;                                       // (e <= 127 - 2 + 1: no clamp above)
}

// the code of v (its fp32 bits) in a cell of scale exponent e; u: the 16 bits of the element
template <int FMT> __host__ __device__ __forceinline__ uint32_t code_of(uint32_t v_bits, int e, uint32_t u) {
    using F = Format<FMT>;
    const uint32_t sign = (v_bits >> 31) << (FMT - 1);
    const Norm n = normalise(v_bits & 0x7fffffffu);
    if (n.sig == 0) return sign;
    const int et = n.x - e;                                           // floor(log2 t)
    const int s = et > F::emin ? et : F::emin;                        // the grid around t has spacing 2^(s - M)
    const int rs = 7 - F::M + (s - et);                               // floor(t 2^(M - s) 2^16) = sig >> rs
    const uint32_t q16 = rs < 32 ? n.sig >> rs : 0u;
    const uint32_t lo = (q16 >> 16) + (static_cast<uint32_t>(s - F::emin) << F::M);
    return sign | (lo + (((q16 & 0xffffu) + u) >> 16));               // (consecutive codes are neighbouring magnitudes; t <= largest: never beyond codemax)
}

// the value of a code under scale byte `scale` (exact; a poisoned cell: NaN)
template <int FMT> __host__ __device__ __forceinline__ float decode(uint32_t code, uint32_t scale) {
    using F = Format<FMT>;
    if (scale == kPoisonScale) return float_of_bits(kNaN);
    const uint32_t mag = code & ((1u << (FMT - 1)) - 1u), field = mag >> F::M, frac = mag & ((1u << F::M) - 1u);
    if (FMT == 8 && mag == 0x7Fu) return float_of_bits(kNaN);
    const int m = static_cast<int>(field != 0 ? frac | (1u << F::M) : frac);
    const int k = (field != 0 ? static_cast<int>(field) - 1 : 0) + F::emin - F::M + static_cast<int>(scale) - 127;
    const float v = ldexpf(static_cast<float>(m), k);
    return (code >> (FMT - 1)) & 1u ? -v : v;
}

// the words of one Philox call: eight consecutive rows (octet 0 .. 3) of column j of block b
__host__ __device__ __forceinline__ void octet_words(size_t b, size_t j, size_t width, int octet, uint32_t domain, Key key, uint32_t (&w)[4]) {
    const uint64_t q = 4 * (static_cast<uint64_t>(b) * width + j) + static_cast<uint64_t>(octet);
    sketch::philox4x32(static_cast<uint32_t>(q), static_cast<uint32_t>(q >> 32), 0u, domain, key, w);
}

// the eight codes of an octet as one little-endian number of 8 FMT bits
template <int FMT> __host__ __device__ __forceinline__ uint64_t octet_codes(const uint32_t (&v_bits)[kBlock], int e, bool poisoned, const uint32_t (&w)[4]) {
    uint64_t word = 0;
#pragma unroll
    for (int r = 0; r < kBlock; ++r) {
        const uint32_t c = poisoned ? (FMT == 8 ? 0x7Fu : 0u) : code_of<FMT>(v_bits[r], e, mask_bits(w, r));
        word |= static_cast<uint64_t>(c) << (FMT * r);
    }
    return word;
}

// ---- the host evaluation, one cell at a time --------------------------------------------------------------------------------------------------
template <int FMT>
inline void pack_cell_host(const float *x, size_t ld, size_t have, size_t b, size_t j, size_t width, uint32_t domain, Key key, uint8_t *scale, uint8_t *cell) {
    uint32_t v[kCellRows], amax = 0;
    bool bad = false;
    for (size_t r = 0; r < static_cast<size_t>(kCellRows); ++r) {
        v[r] = r < have ? bits_of_float(x[r * ld]) : 0u;
        bad = bad || non_finite(v[r]);
        const uint32_t m = v[r] & 0x7fffffffu;
        amax = m > amax ? m : amax;
    }
    const int e = bad ? 128 : scale_of_amax<FMT>(amax);
    *scale = static_cast<uint8_t>(e + 127);
    for (int o = 0; o < kOctets; ++o) {
        uint32_t w[4], vo[kBlock];
        octet_words(b, j, width, o, domain, key, w);
        for (int r = 0; r < kBlock; ++r) vo[r] = v[kBlock * o + r];
        const uint64_t word = octet_codes<FMT>(vo, e, bad, w);
        for (int c = 0; c < FMT; ++c) cell[FMT * o + c] = static_cast<uint8_t>(word >> (8 * c));
    }
}
template <int FMT> inline float decode_cell_host(const uint8_t *cell, uint32_t scale, size_t r) {
    const size_t bit = static_cast<size_t>(FMT) * r;
    const uint32_t two = cell[bit / 8] | (bit / 8 + 1 < cell_bytes(FMT) ? static_cast<uint32_t>(cell[bit / 8 + 1]) << 8 : 0u);
    return decode<FMT>((two >> (bit % 8)) & ((1u << FMT) - 1u), scale);
}

template <class F> bool pick_format(int format, F &&f) { return pick<4, 6, 8>(format, f); }
inline int check_format(const char *name, int format) {
    return known_format(format) ? FEWBIT_OK : fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: format = %d is not 4 (fp4), 6 (fp6) or 8 (fp8)", name, format);
}

}  // namespace mx
}  // namespace fewbit_hip
