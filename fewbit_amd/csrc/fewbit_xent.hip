// fewbit_xent.hip -- the cross entropy of a row of logits against a class index (fewbit_amd/xent.py), on gfx950; part of the companion library
// libfewbit_hipx.so (include/fewbit_hipx.h, "The loss of a row"):
//
//     lse      = log sum_j exp(x_j)
//     loss     = lse - x_t
//     dlogits_j = grow * (exp(x_j - lse) - [j = t])
//
// for logits X (rows x width, F32 / F16 / BF16, row stride ld, no alignment asked of anything) and int64 targets.  Forward reads every element
// once and writes two floats per row; backward reads every element once and writes it once, and may write over the logits.  Nothing but the
// logits themselves and lse has to live between the two.
//
// Arithmetic.  fp32.  exp(a) is v_exp_f32 of a * log2(e): one rounding of the difference, one of the product, the instruction's own.  Forward
// keeps a running (m, s) per lane, s = sum exp(x_j - m) over what the lane has seen: a block of elements gives its maximum first, s is
// rescaled ONCE to max(m, block maximum) and the block's terms are added (a tree of adds).  A block whose maximum is -inf adds nothing and
// rescales nothing -- exp(-inf - (-inf)) is never formed -- unless it holds a NaN, which makes s NaN.  +inf and NaN reach s by themselves
// (inf - inf).  The merge takes the maximum M of the lanes' m first (a butterfly), rescales each lane's s once to M (a lane that has seen
// nothing but -inf gives its s as it is: 0, or NaN) and adds (the same butterfly); the four waves leave (M, s) in LDS and are merged in wave
// order by the same rule.  lse = M + logf(s).  A term is thus rescaled once per block its lane folds afterwards, once to the wave's maximum
// and once to the row's, whatever the width.
//
// Order.  One workgroup of 256 lanes per row at a time, rows taken by the width of the grid (at most kMaxGroups workgroups).  Lane l owns
// element l of the head, the pieces l, l + 256, .. in ascending order and element l of the tail; xor butterfly 32, 16, .. 1; waves 0 .. 3.
// No floating-point atomics: the same arguments give the same bits.
//
// Loads and stores.  A row is walked as [head | 16-byte pieces | tail] (fewbit_moments.hip's span_sum): the head are the elements before the
// first 16-byte boundary, the pieces aligned global_load_dwordx4, the tail what is left behind the last whole piece.  Nothing outside
// [row, row + width) is touched.  Backward stores by the same walk where the output row starts at the same offset from a 16-byte boundary as
// the input row (always so in place); otherwise it walks the row element by element.  Either way an element is read and then written by the
// same lane, so the output may BE the input.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "fewbit_hipx.h"
#include "fewbit_unit.h"

namespace fewbit_hip {
namespace xent {

using unit::fail, unit::check_dtype, unit::pick_dtype, unit::refuse_null, unit::size_of;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr size_t kMaxGroups = 2048;                              // workgroups of either launch: 8 per CU; beyond that a workgroup walks on by the grid's width
constexpr size_t kMaxRows = size_t{1} << 31, kMaxWidth = size_t{1} << 24;          // (rows and the leading dimensions; width)
constexpr float kLog2e = 1.44269504088896340736f;
constexpr uint32_t kNaN = 0x7fc00000u;

// (not fewbit_quantdef.h's Elem: E, the elements of a 16-byte piece, and a widening to float, as fewbit_moments.hip has one to double)
template <int DT> struct Elem { using type = uint16_t; static constexpr int E = 8; };
template <> struct Elem<FEWBIT_F32> { using type = uint32_t; static constexpr int E = 4; };

template <int DT> __device__ __forceinline__ float widen(typename Elem<DT>::type raw) {
    if constexpr (DT == FEWBIT_F32) return __builtin_bit_cast(float, raw);
    else if constexpr (DT == FEWBIT_BF16) return __builtin_bit_cast(float, static_cast<uint32_t>(raw) << 16);
    else return static_cast<float>(__builtin_bit_cast(_Float16, raw));
}
// round to nearest even, as torch's conversions do (a NaN becomes the canonical quiet NaN of bf16)
template <int DT> __device__ __forceinline__ typename Elem<DT>::type narrow(float v) {
    if constexpr (DT == FEWBIT_F32) return __builtin_bit_cast(uint32_t, v);
    else if constexpr (DT == FEWBIT_BF16) {
        const uint32_t bits = __builtin_bit_cast(uint32_t, v);
        if (v != v) return static_cast<uint16_t>(0x7fc0u);
        return static_cast<uint16_t>((bits + 0x7fffu + ((bits >> 16) & 1u)) >> 16);
    } else return __builtin_bit_cast(uint16_t, static_cast<_Float16>(v));
}
template <int DT> __device__ __forceinline__ void unpack(const uint4 &w, float (&v)[Elem<DT>::E]) {
    const uint32_t word[4] = {w.x, w.y, w.z, w.w};
    if constexpr (Elem<DT>::E == 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = widen<DT>(word[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = widen<DT>(static_cast<uint16_t>(word[e >> 1] >> (16 * (e & 1))));
    }
}
template <int DT> __device__ __forceinline__ uint4 pack(const typename Elem<DT>::type (&o)[Elem<DT>::E]) {
    if constexpr (Elem<DT>::E == 4) return uint4{o[0], o[1], o[2], o[3]};
    else
        return uint4{o[0] | static_cast<uint32_t>(o[1]) << 16, o[2] | static_cast<uint32_t>(o[3]) << 16, o[4] | static_cast<uint32_t>(o[5]) << 16,
                     o[6] | static_cast<uint32_t>(o[7]) << 16};
}

// exp(a) for a <= 0 (and NaN, +-inf): v_exp_f32 is 2^x, exact at 0, 0 at -inf
__device__ __forceinline__ float exp_of(float a) { return __builtin_amdgcn_exp2f(a * kLog2e); }

// [head | pieces | tail] of the n elements at p
template <class T> struct Span { size_t head, pieces, tail; };
template <class T> __device__ __forceinline__ Span<T> span_of(const T *p, size_t n) {
    constexpr size_t E = 16 / sizeof(T);
    size_t head = ((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / sizeof(T);
    head = head < n ? head : n;
    const size_t pieces = (n - head) / E;
    return Span<T>{head, pieces, head + pieces * E};
}

// ---- forward: the running (m, s) of a lane ----------------------------------------------------------------------------------------------------
template <int N> __device__ __forceinline__ void fold(const float (&v)[N], float &m, float &s) {
    float top = v[0];
#pragma unroll
    for (int e = 1; e < N; ++e) top = fmaxf(top, v[e]);                             // (fmaxf drops a NaN: it reaches s through its own term)
    if (top > -INFINITY) {
        const float to = fmaxf(m, top);
        s *= exp_of(m - to);                                                        // (m = -inf: s is 0 or NaN and stays so; m = to: times 1)
        m = to;
        float term[N];
#pragma unroll
        for (int e = 0; e < N; ++e) term[e] = exp_of(v[e] - m);
#pragma unroll
        for (int w = 1; w < N; w *= 2) {
#pragma unroll
            for (int e = 0; e + w < N; e += 2 * w) term[e] += term[e + w];
        }
        s += term[0];
    } else {
        // nothing but -inf and NaN: nothing to add, nothing to rescale; a NaN poisons the sum
        bool poisoned = false;
#pragma unroll
        for (int e = 0; e < N; ++e) poisoned = poisoned || v[e] != v[e];
        if (poisoned) s = __builtin_bit_cast(float, kNaN);
    }
}
// s of a run whose maximum is m, at the maximum `to` >= m of several runs
__device__ __forceinline__ float rescaled(float m, float s, float to) { return m > -INFINITY ? s * exp_of(m - to) : s; }

template <int DT>
__global__ __launch_bounds__(kThreads) void forward_kernel(const void *__restrict__ logits_, size_t rows, size_t width, size_t ld, const int64_t *__restrict__ target,
                                                            int64_t ignore_index, float *__restrict__ lse, float *__restrict__ loss) {
    using T = typename Elem<DT>::type;
    constexpr int E = Elem<DT>::E;
    __shared__ float of_wave[kWaves][2];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    for (size_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const T *p = static_cast<const T *>(logits_) + r * ld;
        const int64_t t = threadIdx.x == 0 ? target[r] : 0;
        const Span<T> sp = span_of(p, width);
        float m = -INFINITY, s = 0.0f;
        if (threadIdx.x < sp.head) {
            const float v[1] = {widen<DT>(p[threadIdx.x])};
            fold<1>(v, m, s);
        }
        const uint4 *q = reinterpret_cast<const uint4 *>(p + sp.head);
        size_t c = threadIdx.x;
        for (; c + kThreads < sp.pieces; c += 2 * kThreads) {                       // two pieces in flight
            const uint4 a = q[c], b = q[c + kThreads];
            if constexpr (E == 4) {
                float v[8], u[4];
                unpack<DT>(a, u);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = u[e];
                unpack<DT>(b, u);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[4 + e] = u[e];
                fold<8>(v, m, s);
            } else {
                float v[8];
                unpack<DT>(a, v);
                fold<8>(v, m, s);
                unpack<DT>(b, v);
                fold<8>(v, m, s);
            }
        }
        if (c < sp.pieces) {
            float v[E];
            unpack<DT>(q[c], v);
            fold<E>(v, m, s);
        }
        if (sp.tail + threadIdx.x < width) {
            const float v[1] = {widen<DT>(p[sp.tail + threadIdx.x])};
            fold<1>(v, m, s);
        }
        // the lanes: the maximum first, one rescale each, the sum
        float top = m;
#pragma unroll
        for (int d = 32; d >= 1; d /= 2) top = fmaxf(top, __shfl_xor(top, d, 64));
        float sum = rescaled(m, s, top);
#pragma unroll
        for (int d = 32; d >= 1; d /= 2) sum += __shfl_xor(sum, d, 64);
        if (lane == 0) {
            of_wave[wave][0] = top;
            of_wave[wave][1] = sum;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float all = of_wave[0][0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) all = fmaxf(all, of_wave[w][0]);
            float total = rescaled(of_wave[0][0], of_wave[0][1], all);
#pragma unroll
            for (int w = 1; w < kWaves; ++w) total += rescaled(of_wave[w][0], of_wave[w][1], all);
            const float l = all + logf(total);                                       // (all -inf: -inf + log 0 = -inf)
            lse[r] = l;
            float out = 0.0f;
            if (t != ignore_index) {
                if (t < 0 || static_cast<uint64_t>(t) >= width) out = __builtin_bit_cast(float, kNaN);
                else out = l - widen<DT>(p[t]);                                      // (read after the range check)
            }
            loss[r] = out;
        }
        __syncthreads();                                                             // (of_wave is written again for the next row)
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------------
// d = g * (exp(x - lse) - [e == hot]) + 0: the last term turns a -0 (g < 0 times a probability of 0) into +0
template <int DT> __device__ __forceinline__ typename Elem<DT>::type gradient(float x, float l, float g, bool hot) {
    const float prob = exp_of(x - l);
    return narrow<DT>(g * (hot ? prob - 1.0f : prob) + 0.0f);
}

template <int DT>
__global__ __launch_bounds__(kThreads) void backward_kernel(const void *logits_, size_t rows, size_t width, size_t ld, const int64_t *__restrict__ target,
                                                             int64_t ignore_index, const float *__restrict__ lse, const float *__restrict__ grow, size_t grow_stride,
                                                             void *dlogits_, size_t ld_out) {
    using T = typename Elem<DT>::type;
    constexpr int E = Elem<DT>::E;
    for (size_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const T *p = static_cast<const T *>(logits_) + r * ld;                      // (no __restrict__: out may be p)
        T *out = static_cast<T *>(dlogits_) + r * ld_out;
        const int64_t t = target[r];
        const bool ignored = t == ignore_index, valid = t >= 0 && static_cast<uint64_t>(t) < width;
        const bool same = ((reinterpret_cast<uintptr_t>(p) ^ reinterpret_cast<uintptr_t>(out)) & 15) == 0;
        const Span<T> sp = span_of(out, width);                                      // (same: also the span of p)
        uint4 *qo = reinterpret_cast<uint4 *>(out + sp.head);
        if (ignored || !valid) {
            // nothing of the row is read: +0 for an ignored row, NaN for a target out of range
            const T fill = narrow<DT>(__builtin_bit_cast(float, ignored ? 0u : kNaN));
            T o[E];
#pragma unroll
            for (int e = 0; e < E; ++e) o[e] = fill;
            const uint4 w = pack<DT>(o);
            if (threadIdx.x < sp.head) out[threadIdx.x] = fill;
            for (size_t c = threadIdx.x; c < sp.pieces; c += kThreads) qo[c] = w;
            if (sp.tail + threadIdx.x < width) out[sp.tail + threadIdx.x] = fill;
            continue;
        }
        const float l = lse[r], g = grow[r * grow_stride];
        const uint32_t hot = static_cast<uint32_t>(t);
        if (!same) {
            for (size_t j = threadIdx.x; j < width; j += kThreads) out[j] = gradient<DT>(widen<DT>(p[j]), l, g, static_cast<uint32_t>(j) == hot);
            continue;
        }
        if (threadIdx.x < sp.head) out[threadIdx.x] = gradient<DT>(widen<DT>(p[threadIdx.x]), l, g, threadIdx.x == hot);
        const uint4 *qi = reinterpret_cast<const uint4 *>(p + sp.head);
#pragma unroll 2
        for (size_t c = threadIdx.x; c < sp.pieces; c += kThreads) {
            float v[E];
            unpack<DT>(qi[c], v);
            const uint32_t at = hot - static_cast<uint32_t>(sp.head + c * E);        // (the hot element's place in this piece, if below E)
            T o[E];
#pragma unroll
            for (int e = 0; e < E; ++e) o[e] = gradient<DT>(v[e], l, g, at == static_cast<uint32_t>(e));
            qo[c] = pack<DT>(o);
        }
        const size_t j = sp.tail + threadIdx.x;
        if (j < width) out[j] = gradient<DT>(widen<DT>(p[j]), l, g, static_cast<uint32_t>(j) == hot);
    }
}

inline unsigned grid_of(size_t rows) { return static_cast<unsigned>(rows < kMaxGroups ? rows : kMaxGroups); }

// what both launches refuse alike, in this order
inline int check_rows(const char *name, int dtype, size_t rows, size_t width, size_t ld) {
    if (const int rc = check_dtype(name, dtype)) return rc;
    if (rows == 0 || rows > kMaxRows) return fail(FEWBIT_ERR_UNSUPPORTED, "%s: rows = %zu has no kernel (1 .. %zu rows)", name, rows, kMaxRows);
    if (width == 0 || width > kMaxWidth) return fail(FEWBIT_ERR_UNSUPPORTED, "%s: width = %zu has no kernel (1 .. %zu classes)", name, width, kMaxWidth);
    if (ld < width) return fail(FEWBIT_ERR_UNSUPPORTED, "%s: ld = %zu < width = %zu", name, ld, width);
    if (ld > kMaxRows) return fail(FEWBIT_ERR_UNSUPPORTED, "%s: ld = %zu is beyond %zu", name, ld, kMaxRows);
    return FEWBIT_OK;
}
// the bytes from the first element of the first row to the last of the last one (rows, ld <= 2^31: below 2^65)
inline unsigned __int128 extent(size_t rows, size_t width, size_t ld, size_t element) {
    return (static_cast<unsigned __int128>(rows - 1) * ld + width) * element;
}

}  // namespace xent
}  // namespace fewbit_hip

using namespace fewbit_hip;
using namespace fewbit_hip::xent;

extern "C" {

int fewbit_hipx_cross_entropy_host(const float *logits_host, const int64_t *target_host, size_t rows, size_t width, int64_t ignore_index, const double *grow_host,
                                   double *lse_host, double *loss_host, double *dlogits_host) {
    const char *name = "cross_entropy_host";
    if (rows == 0 || rows > kMaxRows) return fail(FEWBIT_ERR_UNSUPPORTED, "%s: rows = %zu has no kernel (1 .. %zu rows)", name, rows, kMaxRows);
    if (width == 0 || width > kMaxWidth) return fail(FEWBIT_ERR_UNSUPPORTED, "%s: width = %zu has no kernel (1 .. %zu classes)", name, width, kMaxWidth);
    if (logits_host == nullptr || target_host == nullptr || lse_host == nullptr || loss_host == nullptr) return refuse_null(name);
    const double nan = std::nan("");
    for (size_t r = 0; r < rows; ++r) {
        const float *x = logits_host + r * width;
        double top = -INFINITY;
        for (size_t j = 0; j < width; ++j) top = x[j] > top ? x[j] : top;
        double sum = 0.0;
        if (top > -INFINITY)
            for (size_t j = 0; j < width; ++j) sum += std::exp(static_cast<double>(x[j]) - top);          // (+inf, NaN: NaN by themselves)
        else
            for (size_t j = 0; j < width; ++j) sum += x[j] != x[j] ? nan : 0.0;
        const double l = top + std::log(sum);
        const int64_t t = target_host[r];
        const bool ignored = t == ignore_index, valid = t >= 0 && static_cast<uint64_t>(t) < width;
        lse_host[r] = l;
        loss_host[r] = ignored ? 0.0 : valid ? l - static_cast<double>(x[t]) : nan;
        if (dlogits_host == nullptr) continue;
        const double g = grow_host == nullptr ? 1.0 : grow_host[r];
        double *d = dlogits_host + r * width;
        for (size_t j = 0; j < width; ++j)
            d[j] = ignored ? 0.0 : !valid ? nan : g * (std::exp(static_cast<double>(x[j]) - l) - (j == static_cast<size_t>(t) ? 1.0 : 0.0)) + 0.0;
    }
    return FEWBIT_OK;
}

int fewbit_hipx_cross_entropy_forward(int dtype, const void *logits, size_t rows, size_t width, size_t ld, const int64_t *target, int64_t ignore_index, float *lse,
                                      float *loss, void *stream) {
    const char *name = "cross_entropy_forward";
    if (const int rc = check_rows(name, dtype, rows, width, ld)) return rc;
    if (logits == nullptr || target == nullptr || lse == nullptr || loss == nullptr) return refuse_null(name);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_of(rows)), block(kThreads);
    pick_dtype(dtype, [&](auto dt) {
        hipLaunchKernelGGL(forward_kernel<decltype(dt)::value>, grid, block, 0, s, logits, rows, width, ld, target, ignore_index, lse, loss);
    });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

int fewbit_hipx_cross_entropy_backward(int dtype, const void *logits, size_t rows, size_t width, size_t ld, const int64_t *target, int64_t ignore_index,
                                       const float *lse, const float *grow, size_t grow_stride, void *dlogits, size_t ld_out, void *stream) {
    const char *name = "cross_entropy_backward";
    if (const int rc = check_rows(name, dtype, rows, width, ld)) return rc;
    if (ld_out < width) return fail(FEWBIT_ERR_UNSUPPORTED, "%s: ld_out = %zu < width = %zu", name, ld_out, width);
    if (ld_out > kMaxRows) return fail(FEWBIT_ERR_UNSUPPORTED, "%s: ld_out = %zu is beyond %zu", name, ld_out, kMaxRows);
    if (grow_stride > 1) return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: grow_stride = %zu is neither 0 (one scalar) nor 1 (one per row)", name, grow_stride);
    if (logits == nullptr || target == nullptr || lse == nullptr || grow == nullptr || dlogits == nullptr) return refuse_null(name);
    if (!(dlogits == logits && ld_out == ld)) {
        const auto in = reinterpret_cast<uintptr_t>(logits), out = reinterpret_cast<uintptr_t>(dlogits);
        const unsigned __int128 in_end = in + extent(rows, width, ld, size_of(dtype)), out_end = out + extent(rows, width, ld_out, size_of(dtype));
        if (in < out_end && out < in_end)
            return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: dlogits overlaps logits without being logits (in place: the same pointer and ld_out = ld)", name);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_of(rows)), block(kThreads);
    pick_dtype(dtype, [&](auto dt) {
        hipLaunchKernelGGL(backward_kernel<decltype(dt)::value>, grid, block, 0, s, logits, rows, width, ld, target, ignore_index, lse, grow, grow_stride, dlogits,
                           ld_out);
    });
    return hipGetLastError() == hipSuccess ? FEWBIT_OK : fail(FEWBIT_ERR_LAUNCH, "%s: the launch failed", name);
}

}  // extern "C"
