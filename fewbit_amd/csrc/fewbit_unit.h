// fewbit_unit.h -- what a unit of the companion library libfewbit_hipx.so shares with the others: the error reporter, the dtype and pointer
// predicates, the mask of a seed, the plan of a flat sweep, the refusals every entry point words alike and the dispatcher of compile-time choices.
// The units of libfewbit_hip.so take the predicates (known_dtype, size_of) and the dispatcher (pick, pick_dtype) from here too, through fewbit_core.h,
// but none of the refusals: those report through dft::fail, and that library has a reporter and wordings of its own.
// Host code and constants only, beyond the one-line mask_bits: the kernels' bodies stay in their units (routing a kernel through a shared
// __device__ function changes its code, EXPERIMENTS.md 8.16 and 8.27).  Included by fewbit_quantdef.h and fewbit_fft4.h and by the units that
// include neither.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "fewbit_hip.h"

#define FEWBIT_HIDDEN __attribute__((visibility("hidden")))

namespace fewbit_hip {
namespace dft {
// defined by fewbit_dft.hip (g_last_error: what fewbit_hipx_last_error returns); the units of libfewbit_hip.so keep a reporter of their own
FEWBIT_HIDDEN int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
}
namespace unit {

using dft::fail;

// ---- dtype and pointer predicates ---------------------------------------------------------------------------------------------------------
inline bool known_dtype(int dtype) { return dtype == FEWBIT_F32 || dtype == FEWBIT_F16 || dtype == FEWBIT_BF16; }
inline size_t size_of(int dtype) { return dtype == FEWBIT_F32 ? 4 : 2; }
inline bool misaligned(const void *p, size_t to) { return reinterpret_cast<uintptr_t>(p) % to != 0; }           // (a null pointer is aligned)

// ---- the mask of a seed (include/fewbit_hipx.h): counter word 3 = kMaskDomain, thresholds in units of 2^-16 ----------------------------------
constexpr uint32_t kMaskDomain = 5u;        // (0 and 2: the dense sketches, 3: the sampled rows, 4: the CRS columns, 6: the signs, 7 and 8: the rounding)
constexpr uint32_t kOne = 65536u;
// the 16 bits of element e of a block of eight: word e >> 1, low half for even e, high half for odd e; kept where they are >= the threshold
__host__ __device__ __forceinline__ uint32_t mask_bits(const uint32_t (&w)[4], int e) { return (w[e >> 1] >> (16 * (e & 1))) & 0xffffu; }
// what a kept element is multiplied by (threshold = kOne drops everything: 0)
inline float scale_of(uint32_t threshold) { return threshold < kOne ? static_cast<float>(65536.0 / static_cast<double>(kOne - threshold)) : 0.0f; }

// ---- the packed form of a seed, its sizes (the definition itself: fewbit_quantdef.h) -----------------------------------------------------------
constexpr int kBlock = 8;                   // elements per Philox call and per code word
constexpr int kGroup = 64, kLanes = kGroup / kBlock;   // elements per group; lanes that hold one
constexpr size_t kMaxCount = size_t{1} << 36;
// 8 parameter bytes per group, then `bits` code bytes per block (bits: 2, 4 or 8; 1 <= n <= kMaxCount)
inline size_t packed_bytes(size_t n, int bits) { return 8 * ((n + kGroup - 1) / kGroup) + static_cast<size_t>(bits) * ((n + kBlock - 1) / kBlock); }

// ---- the plan of a sweep over a flat tensor (fewbit_quant.hip, fewbit_glu.hip, fewbit_dropout.hip): a lane per block of eight elements,
// workgroups of kThreads lanes, at most kMaxGroups of them; beyond that a lane sweeps on by the grid's width
namespace sweep {
constexpr int kThreads = 256;               // lanes per workgroup
constexpr size_t kMaxGroups = 2048;         // one sweep of the grid: kMaxGroups * kThreads * kBlock = 2^22 elements
static_assert(kThreads % kLanes == 0, "a group's lanes never straddle two sweeps of the grid");
// workgroups for `lanes` lanes of work
inline unsigned grid_of(size_t lanes) {
    const size_t wanted = (lanes + kThreads - 1) / kThreads;
    return static_cast<unsigned>(wanted < kMaxGroups ? wanted : kMaxGroups);
}
}  // namespace sweep

// ---- the refusals that every entry point words alike: FEWBIT_OK, or the status with the message left for fewbit_hipx_last_error ----------------
// (an entry point calls them in the order in which it has always tested its arguments: which refusal a call with two faults gets is behaviour)
inline int check_dtype(const char *name, int dtype) {
    return known_dtype(dtype) ? FEWBIT_OK : fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: unknown dtype %d", name, dtype);
}
inline int check_count(const char *name, size_t n) {
    return n <= kMaxCount ? FEWBIT_OK : fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: n = %zu is beyond 2^36", name, n);
}
inline int refuse_null(const char *name) { return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: null pointer", name); }
inline int check_seed_word(const char *name, const void *seed_device) {
    return !misaligned(seed_device, 8) ? FEWBIT_OK : fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: the seed word in device memory must be 8-byte aligned", name);
}
// `what`: "state", "out", "packed"
inline int check_aligned8(const char *name, const char *what, const void *p) {
    return !misaligned(p, 8) ? FEWBIT_OK : fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: %s must be 8-byte aligned", name, what);
}
// `what`: "state", "out", "the workspace"
inline int check_bytes(const char *name, const char *what, size_t have, size_t need) {
    return have >= need ? FEWBIT_OK : fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s: %s has %zu bytes, %zu are needed", name, what, have, need);
}

// ---- one dispatcher for compile-time choices: f(std::integral_constant<int, V>{}) for the V of VS that equals v; false (and no call) for none ---
template <int V, int... VS, class F> bool pick(int v, F &&f) {
    if (v == V) return f(std::integral_constant<int, V>{}), true;
    if constexpr (sizeof...(VS) != 0) return pick<VS...>(v, f);
    else return false;
}
template <class F> bool pick_dtype(int dtype, F &&f) { return pick<FEWBIT_F32, FEWBIT_F16, FEWBIT_BF16>(dtype, f); }

}  // namespace unit
}  // namespace fewbit_hip
