// unit_host_check.cpp -- drives the host code of fewbit_amd/csrc/fewbit_unit.h (and check_bits of fewbit_quantdef.h) the way the entry points of
// libfewbit_hipx.so do: every shared refusal with values it takes and values it refuses, the wording of each message, the predicates, the plan of a
// sweep, the packed size, scale_of and mask_bits at their edges, and pick with every value of its list and with values outside it.  It brings its own
// fewbit_hip::dft::fail (the library's lives in fewbit_dft.hip).  Meant for a sanitizer build of the host code alone (no GPU, no HIP runtime):
//
//     hipcc -x hip --cuda-host-only -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -I include -I fewbit_amd/csrc \
//         tools/unit_host_check.cpp -o unit_host_check && ./unit_host_check
//
// Exit status 0 and "ok" when every expectation holds.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fewbit_quantdef.h"

static char g_message[256] = "";
namespace fewbit_hip {
namespace dft {
int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_message, sizeof g_message, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace dft
}  // namespace fewbit_hip

using namespace fewbit_hip;
using namespace fewbit_hip::unit;

static long g_bad = 0, g_checks = 0;
static void expect(bool ok, const char *what) {
    ++g_checks;
    if (!ok) ++g_bad, std::printf("FAILED: %s (last message: %s)\n", what, g_message);
}
// a refusal: the status and the message, byte for byte
static void refused(int status, const char *message) { expect(status == FEWBIT_ERR_INVALID_ARGUMENT && std::strcmp(g_message, message) == 0, message); }

int main() {
    const void *const aligned = reinterpret_cast<const void *>(uintptr_t{0x10000});
    const auto at = [&](size_t off) { return reinterpret_cast<const void *>(uintptr_t{0x10000} + off); };

    for (int dtype : {FEWBIT_F32, FEWBIT_F16, FEWBIT_BF16}) expect(known_dtype(dtype) && check_dtype("f", dtype) == FEWBIT_OK, "a known dtype");
    for (int dtype : {-1, 3, 1 << 30}) expect(!known_dtype(dtype) && check_dtype("f", dtype) == FEWBIT_ERR_INVALID_ARGUMENT, "an unknown dtype");
    refused(check_dtype("quant_pack", 7), "quant_pack: unknown dtype 7");
    expect(size_of(FEWBIT_F32) == 4 && size_of(FEWBIT_F16) == 2 && size_of(FEWBIT_BF16) == 2, "size_of");

    for (int bits : {2, 4, 8}) expect(quant::check_bits("f", bits) == FEWBIT_OK, "known bits");
    for (int bits : {-8, 0, 1, 3, 5, 6, 7, 9, 16, 1 << 30}) expect(quant::check_bits("f", bits) == FEWBIT_ERR_INVALID_ARGUMENT, "unknown bits");
    refused(quant::check_bits("glu_forward", 3), "glu_forward: bits = 3 is not 2, 4 or 8");

    expect(!misaligned(nullptr, 16) && !misaligned(aligned, 16), "aligned pointers");
    for (size_t off : {1, 2, 4, 8}) expect(misaligned(at(off), 16) && misaligned(at(off), 8) == (off < 8) && misaligned(at(off), 4) == (off < 4), "misaligned pointers");
    expect(check_seed_word("f", nullptr) == FEWBIT_OK && check_seed_word("f", at(8)) == FEWBIT_OK, "a seed word that is absent or aligned");
    refused(check_seed_word("dropout", at(4)), "dropout: the seed word in device memory must be 8-byte aligned");
    expect(check_aligned8("f", "state", nullptr) == FEWBIT_OK && check_aligned8("f", "state", at(8)) == FEWBIT_OK, "a state that is absent or aligned");
    refused(check_aligned8("rms_norm_backward", "state", at(1)), "rms_norm_backward: state must be 8-byte aligned");
    refused(check_aligned8("quant_unpack", "packed", at(4)), "quant_unpack: packed must be 8-byte aligned");

    expect(check_count("f", 0) == FEWBIT_OK && check_count("f", kMaxCount) == FEWBIT_OK, "counts up to 2^36");
    refused(check_count("quant_unpack_host", kMaxCount + 1), "quant_unpack_host: n = 68719476737 is beyond 2^36");
    expect(check_count("f", ~size_t{0}) == FEWBIT_ERR_INVALID_ARGUMENT, "the largest count");
    expect(check_bytes("f", "state", 660, 660) == FEWBIT_OK && check_bytes("f", "state", 0, 0) == FEWBIT_OK, "enough bytes");
    refused(check_bytes("layer_norm_forward", "state", 659, 660), "layer_norm_forward: state has 659 bytes, 660 are needed");
    refused(check_bytes("rms_norm_backward", "the workspace", 0, 8192), "rms_norm_backward: the workspace has 0 bytes, 8192 are needed");
    refused(refuse_null("glu_state_host"), "glu_state_host: null pointer");

    expect(packed_bytes(1, 2) == 8 + 2 && packed_bytes(64, 4) == 8 + 32 && packed_bytes(65, 8) == 16 + 72, "packed_bytes at the edges of a group");
    expect(packed_bytes(kMaxCount, 8) == kMaxCount / 8 + kMaxCount, "packed_bytes of the largest count");
    expect(sweep::grid_of(0) == 0 && sweep::grid_of(1) == 1 && sweep::grid_of(256) == 1 && sweep::grid_of(257) == 2, "grid_of at the edges of a workgroup");
    expect(sweep::grid_of(sweep::kMaxGroups * sweep::kThreads + 1) == sweep::kMaxGroups && sweep::grid_of(kMaxCount) == sweep::kMaxGroups, "grid_of at its ceiling");

    expect(scale_of(0) == 1.0f && scale_of(32768) == 2.0f && scale_of(kOne - 1) == 65536.0f && scale_of(kOne) == 0.0f && scale_of(~0u) == 0.0f, "scale_of");
    const uint32_t words[4] = {0x00010000u, 0xffff8000u, 0x12345678u, 0x0000ffffu};
    const uint32_t want[8] = {0x0000u, 0x0001u, 0x8000u, 0xffffu, 0x5678u, 0x1234u, 0xffffu, 0x0000u};
    for (int e = 0; e < 8; ++e) expect(mask_bits(words, e) == want[e] && quant::uniform_of(words, e) == static_cast<float>(want[e]) / 65536.0f, "mask_bits / uniform_of");

    // pick: the one value, in the order of the list, nothing for a value outside it
    std::vector<int> seen;
    for (int v : {2, 4, 8}) expect(pick<2, 4, 8>(v, [&](auto c) { seen.push_back(decltype(c)::value); }), "pick takes a value of its list");
    expect(seen == std::vector<int>({2, 4, 8}), "pick passes the value on");
    for (int v : {-1, 0, 1, 3, 16, 1 << 30}) expect(!pick<2, 4, 8>(v, [&](auto) { seen.push_back(-1); }), "pick refuses a value outside its list");
    expect(seen.size() == 3, "pick calls nothing for a value outside its list");
    expect(pick<1, 0>(true, [&](auto c) { expect(decltype(c)::value == 1, "true is 1"); }) && pick<1, 0>(false, [&](auto c) { expect(decltype(c)::value == 0, "false is 0"); }),
           "pick on a bool");
    expect(pick<7>(7, [](auto) {}) && !pick<7>(8, [](auto) {}), "pick with one value");
    std::string path;
    for (int dtype : {0, 1, 2, 3})
        pick_dtype(dtype, [&](auto dt) { pick<0, 2, 4, 8>(4, [&](auto b) { path += std::to_string(decltype(dt)::value) + ":" + std::to_string(decltype(b)::value) + " "; }); });
    expect(path == "0:4 1:4 2:4 ", "nested picks");

    std::printf("%s: %ld checks, %ld failed\n", g_bad == 0 ? "ok" : "FAILED", g_checks, g_bad);
    return g_bad == 0 ? 0 : 1;
}
