// fewbit_core.h -- what the units of libfewbit_hip.so (fewbit_kernels.hip, fewbit_sketch.hip, fewbit_dct.hip) share: the error reporter, the hand-over of
// a tune key to the sketch unit and the cached CU count of a device; and the host helpers of the activation unit that are checked on their own, without a
// device (tools/core_host_check.cpp): the launch shape of a streaming kernel and the check of a call's buffers.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <initializer_list>

#include "fewbit_unit.h"

namespace fewbit_hip {

// defined by the core unit of fewbit_kernels.hip (g_last_error: what fewbit_hip_last_error returns)
extern FEWBIT_HIDDEN thread_local char g_last_error[256];
FEWBIT_HIDDEN int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// defined by fewbit_sketch.hip: the keys of fewbit_hip_tune that belong to that unit
FEWBIT_HIDDEN int sketch_tune(const char *key, long long value, bool *known);

// ---- the CU count of device `dev` (0 <= dev < kMaxDevices), asked once per device; 256 where the runtime does not say --------------------------
// (what a caller does without a current device is its own: open_call of the activation unit refuses, device_cus of the sketch unit takes 256)
constexpr int kMaxDevices = 64;
inline int cached_cus(int dev) {
    static std::atomic<int> cus[kMaxDevices];
    int v = cus[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) {
            (void)hipGetLastError();
            v = 256;
        }
        cus[dev].store(v, std::memory_order_relaxed);     // (two threads racing on a first use store the same value)
    }
    return v;
}

// ---- the launch shape of a streaming kernel (see Span in fewbit_kernels.hip) --------------------------------------------------------------------
// RESIDENT (chunk = 0: one wave per tile until the chip is full, then the resident waves loop round-robin) or CHUNKED (chunk = T tiles per wave,
// block-contiguous, as many blocks as that takes).
struct Shape { unsigned blocks; int chunk; };

// Built-in policy (measured on MI355X, scratch/headvar.py with SIZES=..., EXPERIMENTS.md section 6): the resident shape wins
// while a wave has only a few tiles (4096x4096 bf16: 11.2 vs 11.6 us), the chunked shape wins once the tensor is many
// times the resident generation, where statically assigned waves drift apart and the launch waits for the slowest
// (2^28 bf16 elements: backward 235 -> 197 us, pattern-table forward 224 -> 197 us; RoBERTa-size fp32, 5*10^7 elements:
// forward+backward 169 -> 151 us).  `min_ratio` = tiles per resident wave from which the chunked shape is used.
// `setting`: -1 = that policy, 0 = always resident, T = chunk of T wherever the tensor has more tiles than resident waves.
inline Shape launch_shape(size_t ntiles, int waves_per_block, size_t resident_blocks, long long setting, int auto_chunk, size_t min_ratio) {
    const size_t wpb = static_cast<size_t>(waves_per_block);
    size_t blocks = (ntiles + wpb - 1) / wpb;                      // one tile per wave
    int chunk = 0;
    if (blocks > resident_blocks) {
        long long t = setting;
        if (t < 0) t = ntiles >= min_ratio * resident_blocks * wpb ? auto_chunk : 0;
        const size_t chunked = t > 0 ? (ntiles + wpb * t - 1) / (wpb * t) : 0;
        if (t > 0 && chunked > resident_blocks) {
            blocks = chunked;
            chunk = static_cast<int>(t);
        } else {
            blocks = resident_blocks;
        }
    }
    if (blocks < 1) blocks = 1;
    return Shape{static_cast<unsigned>(blocks), chunk};
}

// ---- the buffers of a call ----------------------------------------------------------------------------------------------------------------------
// FEWBIT_HIP_VALIDATE=1 (debug aid, off by default: two runtime queries per pointer): every pointer handed to the
// C-ABI must be device memory and [p, p + bytes) must lie inside its allocation -- a host pointer or a state buffer
// sized with the wrong bit width then fails with FEWBIT_ERR_INVALID_ARGUMENT instead of a fault on the GPU.
inline bool validate_enabled() {
    static const bool on = [] {
        const char *e = getenv("FEWBIT_HIP_VALIDATE");
        return e && atoi(e) != 0;
    }();
    return on;
}

inline int validate_range(const char *what, const void *p, size_t bytes) {
    if (!validate_enabled() || bytes == 0) return FEWBIT_OK;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s (%p) is not a pointer known to the HIP runtime", what, p);
    }
    if (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged)
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s (%p) is not device memory", what, p);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s (%p): no allocation found", what, p);
    }
    const size_t off = static_cast<size_t>(static_cast<const char *>(p) - static_cast<const char *>(base));
    if (off + bytes > size)
        return fail(FEWBIT_ERR_INVALID_ARGUMENT, "%s needs %zu bytes but only %zu remain in its allocation", what, bytes, size - off);
    return FEWBIT_OK;
}

// The one argument check behind every entry point that launches: true where the call ends here with *rc -- FEWBIT_OK for n == 0 (no pointer is looked
// at), a refusal for a null pointer (any of them, before any range) or, under FEWBIT_HIP_VALIDATE, for the first buffer of the list that is not
// `bytes` of device memory.  (What an entry point tests before its buffers -- table size, dtype, fn, bit width -- and after them stays in its own
// order there: which refusal a call with two faults gets is behaviour.)
struct Buffer { const char *name; const void *p; size_t bytes; };
inline bool ends_at_buffers(int *rc, size_t n, std::initializer_list<Buffer> buffers) {
    *rc = FEWBIT_OK;
    if (n == 0) return true;
    for (const Buffer &b : buffers)
        if (!b.p) return *rc = fail(FEWBIT_ERR_INVALID_ARGUMENT, "null pointer argument"), true;
    for (const Buffer &b : buffers)
        if ((*rc = validate_range(b.name, b.p, b.bytes)) != FEWBIT_OK) return true;
    return false;
}

}  // namespace fewbit_hip
