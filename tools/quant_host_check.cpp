// quant_host_check.cpp -- drives the two host functions of fewbit_amd/csrc/fewbit_quantdef.h (pack_group_host, decode_host) through exactly
// sized heap buffers, the way the four *_host entry points of libfewbit_hipx.so loop over them: flat tensors and rows of a state, every group
// count 1 .. 64, the last partial block of every width, 2 / 4 / 8 bits, two seeds, normal, constant, NaN- and inf-holding values.  Meant for a
// sanitizer build of the host code alone (no GPU, no HIP runtime):
//
//     hipcc -x hip --cuda-host-only -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I include -I fewbit_amd/csrc \
//         tools/quant_host_check.cpp -o quant_host_check && ./quant_host_check
//
// Exit status 0 and "ok" when every finite element decodes within one step of its value and every poisoned group to NaN.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fewbit_quantdef.h"

using namespace fewbit_hip;
using namespace fewbit_hip::quant;

static std::vector<float> values(size_t n, int kind, uint32_t salt) {
    std::vector<float> x(n);
    uint32_t s = 12345u + salt;
    for (size_t i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        x[i] = kind == 1 ? 3.25f : static_cast<float>(static_cast<int32_t>(s >> 8) % 4096 - 2048) / 512.0f;
    }
    if (kind == 2) x[n / 2] = NAN;
    if (kind == 3) x[n / 3] = INFINITY;
    return x;
}

// `rows` rows of `width` elements, groups and blocks per row (the layout of a state; rows = 1 with stride = the code bytes: a flat tensor)
static long check(size_t rows, size_t width, int bits, uint64_t seed, int kind) {
    const size_t groups = (width + kGroup - 1) / kGroup, blocks = (width + kBlock - 1) / kBlock, stride = static_cast<size_t>(bits) * blocks;
    const std::vector<float> x = values(rows * width, kind, static_cast<uint32_t>(width));
    uint8_t *out = static_cast<uint8_t *>(std::malloc(rows * (8 * groups + stride)));
    const Key key = sketch::key_of(seed);
    long bad = 0;
    for (size_t r = 0; r < rows; ++r) {
        uint8_t *codes = out + 8 * rows * groups + r * stride;
        for (size_t g = 0; g < groups; ++g) {
            const size_t first = g * kGroup, count = width - first < static_cast<size_t>(kGroup) ? width - first : kGroup;
            pack_group_host(x.data() + r * width + first, count, r * blocks + g * kLanes, key, bits, out + 8 * (r * groups + g),
                            codes + static_cast<size_t>(bits) * kLanes * g);
        }
        for (size_t i = 0; i < width; ++i) {
            const uint8_t *par = out + 8 * (r * groups + i / kGroup);
            uint32_t step_bits;
            std::memcpy(&step_bits, par + 4, 4);
            const float step = float_of_bits(step_bits), got = decode_host(out + 8 * r * groups, codes, i, bits), want = x[r * width + i];
            bool poisoned = false;
            for (size_t j = i / kGroup * kGroup; j < width && j < (i / kGroup + 1) * kGroup; ++j) poisoned = poisoned || !std::isfinite(x[r * width + j]);
            bad += poisoned ? !(got != got) : !(std::fabs(got - want) <= step * (1.0f + 1.0f / 1048576.0f));
        }
    }
    std::free(out);
    return bad;
}

int main() {
    const size_t sizes[] = {1, 7, 8, 9, 63, 64, 65, 205, 2573}, widths[] = {1, 3, 7, 8, 9, 63, 64, 65, 200, 770};
    const uint64_t seeds[] = {0x1234567887654321ull, 7};
    long bad = 0, calls = 0;
    for (int bits : {2, 4, 8})
        for (uint64_t seed : seeds)
            for (int kind = 0; kind < 4; ++kind) {
                for (size_t n : sizes) bad += check(1, n, bits, seed, kind), ++calls;
                for (size_t width : widths) bad += check(3, width, bits, seed, kind), ++calls;
                for (size_t count = 1; count <= static_cast<size_t>(kGroup); ++count) bad += check(2, count, bits, seed, kind), ++calls;
                for (size_t width = 1; width <= 4 * static_cast<size_t>(kGroup); ++width) bad += check(1, width, bits, seed, kind), ++calls;
            }
    std::printf("%s: %ld layouts, %ld elements out of bound\n", bad == 0 ? "ok" : "FAILED", calls, bad);
    return bad == 0 ? 0 : 1;
}
