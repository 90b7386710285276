// core_host_check.cpp -- drives the host helpers of fewbit_amd/csrc/fewbit_core.h the way the activation unit (fewbit_kernels.hip) does: launch_shape at
// the edges of its policy and the check of a call's buffers with each fault, in each order.  It brings its own fewbit_hip::fail (the library's lives in
// the core unit of fewbit_kernels.hip).  Meant for a sanitizer build of the host code alone, run without a GPU:
//
//     hipcc -x hip --cuda-host-only -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -I include -I fewbit_amd/csrc \
//         tools/core_host_check.cpp -o core_host_check && ./core_host_check && FEWBIT_HIP_VALIDATE=1 HIP_VISIBLE_DEVICES=-1 ./core_host_check
//
// (the second run: the range check of every buffer, which asks the runtime and, with no device to be seen, knows none of the pointers).
// Exit status 0 and "ok" when every expectation holds.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "fewbit_core.h"

static char g_message[256] = "";
namespace fewbit_hip {
int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_message, sizeof g_message, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace fewbit_hip

using namespace fewbit_hip;

static long g_bad = 0, g_checks = 0;
static void expect(bool ok, const char *what) {
    ++g_checks;
    if (!ok) ++g_bad, std::printf("FAILED: %s (last message: %s)\n", what, g_message);
}
static bool is(Shape s, unsigned blocks, int chunk) { return s.blocks == blocks && s.chunk == chunk; }

int main() {
    // ---- launch_shape: 4 waves per block, R resident blocks, so 4 R tiles fill the chip with one tile per wave ----
    const size_t R = 512, full = 4 * R;
    for (long long setting : {-1ll, 0ll, 3ll}) {
        expect(is(launch_shape(0, 4, R, setting, 1, 4), 1, 0), "no tile: one block (of the tail), resident");
        expect(is(launch_shape(1, 4, R, setting, 1, 4), 1, 0), "one tile: one block");
        expect(is(launch_shape(5, 4, R, setting, 1, 4), 2, 0), "five tiles: two blocks");
        expect(is(launch_shape(full, 4, R, setting, 1, 4), R, 0), "exactly the resident count: resident, every wave one tile");
    }
    // one tile more than fits: the policy stays resident below `min_ratio` tiles per resident wave, 0 always, T chunks wherever that needs more blocks than fit
    expect(is(launch_shape(full + 1, 4, R, -1, 1, 4), R, 0), "one more, policy: resident");
    expect(is(launch_shape(full + 1, 4, R, 0, 1, 4), R, 0), "one more, setting 0: resident");
    expect(is(launch_shape(full + 1, 4, R, 1, 1, 4), R + 1, 1), "one more, setting 1: chunked, one block more");
    expect(is(launch_shape(full + 1, 4, R, 3, 1, 4), R, 0), "one more, setting 3: the chunked grid would not fill the chip, resident");
    expect(is(launch_shape(3 * full, 4, R, 3, 1, 4), R, 0), "three per wave, setting 3: exactly the resident count of blocks, resident");
    expect(is(launch_shape(3 * full + 1, 4, R, 3, 1, 4), R + 1, 3), "one more than that: chunked");
    expect(is(launch_shape(4 * full - 1, 4, R, -1, 1, 4), R, 0), "policy, just below the ratio: resident");
    expect(is(launch_shape(4 * full, 4, R, -1, 1, 4), 4 * R, 1), "policy, at the ratio: one tile per wave");
    expect(is(launch_shape(12 * 16 * R - 1, 16, R, -1, 3, 12), R, 0), "table class, just below its ratio: resident");
    expect(is(launch_shape(12 * 16 * R, 16, R, -1, 3, 12), 4 * R, 3), "table class, at its ratio: three tiles per wave");
    expect(is(launch_shape(size_t{1} << 32, 4, R, -1, 1, 4), 1u << 30, 1), "a grid of 2^30 blocks");
    expect(is(launch_shape(7, 4, 0, -1, 1, 4), 2, 1) && is(launch_shape(7, 4, 0, 0, 1, 4), 1, 0), "nothing resident (never asked for): no division by it");

    // ---- ends_at_buffers ----
    const bool validating = validate_enabled();
    const void *const p = reinterpret_cast<const void *>(uintptr_t{0x10000});
    int rc = 77;
    expect(ends_at_buffers(&rc, 0, {{"x", nullptr, 0}, {"y", nullptr, 0}}) && rc == FEWBIT_OK, "n = 0 ends the call with FEWBIT_OK and looks at no pointer");
    expect(ends_at_buffers(&rc, 0, {}) && rc == FEWBIT_OK, "n = 0 and no buffer");
    for (int null_at = 0; null_at < 4; ++null_at) {
        g_message[0] = 0;
        const void *q[4] = {p, p, p, p};
        q[null_at] = nullptr;
        expect(ends_at_buffers(&rc, 8, {{"x", q[0], 16}, {"y", q[1], 16}, {"state", q[2], 3}, {"borders", q[3], 30}}) && rc == FEWBIT_ERR_INVALID_ARGUMENT &&
                   std::strcmp(g_message, "null pointer argument") == 0,
               "a null pointer at any place of the list is refused, before any range");
    }
    g_message[0] = 0;
    expect(ends_at_buffers(&rc, 8, {{"x", nullptr, 16}, {"state", nullptr, 3}}) && rc == FEWBIT_ERR_INVALID_ARGUMENT, "two null pointers");
    g_message[0] = 0;
    const bool ended = ends_at_buffers(&rc, 8, {{"codes", p, 32}, {"state", p, 4}});
    if (!validating) {
        expect(!ended && rc == FEWBIT_OK && g_message[0] == 0, "no null pointer: the call goes on, nothing is reported");
    } else {
        expect(ended && rc == FEWBIT_ERR_INVALID_ARGUMENT && std::strcmp(g_message, "codes (0x10000) is not a pointer known to the HIP runtime") == 0,
               "validating: the first buffer of the list that is not device memory");
        expect(ends_at_buffers(&rc, 8, {{"state", p, 4}, {"codes", p, 32}}) && std::strcmp(g_message, "state (0x10000) is not a pointer known to the HIP runtime") == 0,
               "validating: in the order of the list");
        expect(ends_at_buffers(&rc, 8, {{"state", p, 0}, {"codes", p, 32}}) && std::strcmp(g_message, "codes (0x10000) is not a pointer known to the HIP runtime") == 0,
               "validating: a buffer of no bytes is not asked about");
        expect(ends_at_buffers(&rc, 8, {{"x", p, 16}, {"y", nullptr, 16}}) && std::strcmp(g_message, "null pointer argument") == 0, "validating: a null pointer wins over a range");
        expect(!ends_at_buffers(&rc, 8, {{"state", p, 0}}) && rc == FEWBIT_OK, "validating: nothing to ask");
    }

    std::printf("%s: %ld checks, %ld failed%s\n", g_bad == 0 ? "ok" : "FAILED", g_checks, g_bad, validating ? " (FEWBIT_HIP_VALIDATE=1)" : "");
    return g_bad == 0 ? 0 : 1;
}
