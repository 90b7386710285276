#!/usr/bin/env python3
"""The plans of the dense sketch (fewbit_hip_sketch_describe, fewbit_hip_sketch_workspace) as a library build answers them, recorded so that
a later build can be held against them (tests/test_sketch_plan_host.py):

    FEWBIT_HIP_LIB=<libfewbit_hip.so of the commit to record> python tests/golden/gen_sketch_plans.py <that commit>
        ->  tests/golden/sketch_plans.json

The table is made from the commit BEFORE a change of the host side, never from the change itself.  No GPU: without a device the library
plans for 256 CUs (what an MI355X reports); the generator refuses to run where a device is visible and reports another count.

    shapes           (rows, features, proj) listed one by one: every shape tests/test_gpu_sketch.py describes or multiplies, the bench's,
                     both sides of the fragment caps (1 GiB, 65535 row blocks), 2^21 rows, empty calls
    threshold_cross  rows x features x proj around the policy's thresholds: 1024-row slices, 256 / 1024 / 2048 features and the 512-wide
                     tile's divisibility, proj 1280 | 1281, rows long enough for 16 slices of a one-tile grid
    fuzz_cross       the edge lists of test_seeded_fuzz_of_shapes_dtypes_strides_and_tiles
    default          the built-in policy: per distribution / dtype, [describe string as written, workspace bytes] of every listed shape
    settings         per tuning setting (each key alone at its non-default values; sketch_slices takes any count > 0: the ones the tests
                     force, the cap of 16 and beyond; then the combinations the GPU tests use) and distribution / dtype ONE SHA-256 over the
                     lines "rows features proj workspace describe-string" of all three shape sets, in order
    fuzz_cases       the 60 draws of that fuzz test with their six tuning values, answers in full
"""
import json
import random
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE.parents[1])]

import torch  # noqa: E402

from fewbit_amd import cabi  # noqa: E402
from test_sketch_plan_host import DISTS, DTYPES, all_shapes, answers, digest, tune  # noqa: E402

SHAPES = (
    # tests/test_gpu_sketch.py, in the order of the file
    (64, 256, 128), (100, 37, 5), (1000, 264, 130), (257, 8, 1), (4096, 512, 256), (3000, 770, 200), (2048, 1024, 300), (512, 100, 64),
    (16384, 3072, 3276), (16384, 768, 3276), (16384, 768, 1000), (16384, 256, 3276), (2**21, 768, 2**10),
    (5000, 776, 300), (2049, 520, 257), (3000, 384, 1400), (8192, 384, 200), (16384, 3072, 1638),
    (3000, 770, 1400), (520, 264, 1300), (70000, 40, 1290), (300, 1032, 2000), (700, 2056, 1300),
    (8192, 392, 200), (3000, 389, 130), (8192, 392, 1400), (2**20 + 3, 264, 200),
    (16384, 768, 1280), (16384, 768, 1281), (4096, 512, 1400), (2048, 1024, 1300), (1000, 37, 5), (2048, 512, 130),
    (3000, 520, 300), (1111, 1024, 129), (4096, 264, 64), (9000, 768, 700), (512, 48, 64), (512, 64, 96), (300, 40, 24),
    # thresholds one at a time on the bench's layer (the cross product below has them in combination)
    (16384, 3072, 1280), (16384, 3072, 1281), (16384, 256, 1638), (16384, 257, 1638), (16384, 1023, 1638), (16384, 1024, 1638),
    (16384, 1536, 1638), (16384, 1280, 1638), (16384, 2047, 1638), (16384, 2048, 1638), (16384, 2304, 1638), (1023, 768, 200), (1024, 768, 200),
    (2047, 768, 200), (2048, 768, 200), (16384, 256, 128), (65536, 256, 128), (100000, 200, 100), (2**21, 3072, 128),
    # the fragment caps: 1 GiB of fragments (8 row blocks x 8192 | 8191 blocks of 256 rows), 65535 row blocks of S
    (2**21, 768, 256), (2**21 - 256, 768, 256), (256, 512, 2**21), (256, 512, 2**21 - 256),
    # nothing to do
    (0, 16, 4), (16, 0, 4), (16, 8, 0), (0, 0, 0),
)
THRESHOLD_CROSS = ((1023, 1024, 16384, 65536), (256, 257, 1023, 1024, 1536, 2047, 2048, 2304), (128, 1280, 1281, 3276))
FUZZ_EDGES = ((1, 7, 8, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 3000),
              (1, 8, 9, 40, 255, 256, 257, 264, 511, 512, 520, 768, 1032), (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 300))
SETTINGS = ([{}]
            + [{'sketch_slices': z} for z in (1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 17, 1000)]
            + [{'sketch_waves': w} for w in (4, 8)] + [{'sketch_halves': h} for h in (1, 2)] + [{'sketch_convert': c} for c in (0, 1)]
            + [{'sketch_partials': p} for p in (0, 1, 2)] + [{'sketch_materialise': m} for m in (0, 1)]
            # test_gaussian_fragments_from_memory_are_the_fused_kernels_matrix, test_row_slices_are_deterministic_and_agree
            + [{'sketch_slices': z, 'sketch_waves': w, 'sketch_halves': 1, 'sketch_materialise': m} for z in (1, 2, 3) for w in (8, 4) for m in (0, 1)]
            + [{'sketch_halves': 2, 'sketch_materialise': 0}, {'sketch_halves': 1, 'sketch_materialise': 1}, {'sketch_halves': 1, 'sketch_materialise': 0},
               {'sketch_halves': 1, 'sketch_waves': 4}, {'sketch_halves': 1, 'sketch_waves': 8}]
            # test_bf16_partial_sums_of_sliced_bf16_products, test_fp32_input_converted_to_bf16_first_gives_the_same_products
            + [{'sketch_slices': z, 'sketch_partials': p} for z in (2, 4, 7) for p in (0, 1)]
            + [{'sketch_convert': c, 'sketch_partials': 2} for c in (0, 1)] + [{'sketch_convert': 1, 'sketch_slices': 3}])


def fuzz_cases(L):
    """the draws of test_seeded_fuzz_of_shapes_dtypes_strides_and_tiles, stream for stream"""
    rnd, rnd_convert, rnd_partials, rnd_memory = random.Random(20260402), random.Random(7), random.Random(8), random.Random(9)
    cases = []
    for _ in range(60):
        dist = rnd.choice((0, 1))
        dtype = rnd.choice((0, 2, 1))                                  # (torch.float32, torch.bfloat16, torch.float16) as enum fewbit_dtype
        shape = tuple(rnd.choice(edges) for edges in FUZZ_EDGES)
        setting = {'sketch_waves': rnd.choice((-1, 4, 8)), 'sketch_halves': rnd.choice((-1, 1, 2)), 'sketch_slices': rnd.choice((-1, 1, 2, 3)),
                   'sketch_convert': rnd_convert.choice((-1, 0, 1)), 'sketch_partials': rnd_partials.choice((-1, 0, 1)),
                   'sketch_materialise': rnd_memory.choice((-1, 0, 1))}
        if shape[1] > 1:
            rnd.choice((0, 0, 8, 3))                                   # (the row stride, the seed, the scale: drawn to keep the sequence)
        rnd.getrandbits(64)
        rnd.choice((1.0, 1.0 / shape[2], -0.5))
        tune(L, setting)
        text, workspace = answers(L, dist, dtype, shape)
        cases.append({'dist': dist, 'dtype': dtype, 'shape': list(shape), 'tune': setting, 'describe': text, 'workspace': workspace})
    return cases


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        sys.exit('a device with a CU count other than 256 is visible: the table is recorded for 256')
    L = cabi.lib()
    table = {'commit': sys.argv[1], 'cus': 256,
             'recipe': 'tests/golden/gen_sketch_plans.py; digests: sha256 over "rows features proj workspace describe-string\\n" of shapes, then '
                       'the product of threshold_cross, then the product of fuzz_cross',
             'shapes': [list(s) for s in SHAPES], 'threshold_cross': [list(e) for e in THRESHOLD_CROSS], 'fuzz_cross': [list(e) for e in FUZZ_EDGES]}
    shapes = all_shapes(table)
    try:
        tune(L, {})
        table['default'] = {f'{dist}/{dtype}': [list(answers(L, d, t, s)) for s in SHAPES] for d, dist in enumerate(DISTS) for t, dtype in enumerate(DTYPES)}
        table['settings'] = []
        for setting in SETTINGS:
            tune(L, setting)
            table['settings'].append({'tune': setting, 'digests': {f'{dist}/{dtype}': digest(L, d, t, shapes) for d, dist in enumerate(DISTS) for t, dtype in enumerate(DTYPES)}})
        table['fuzz_cases'] = fuzz_cases(L)
    finally:
        tune(L, {})
    (HERE / 'sketch_plans.json').write_text(json.dumps(table, indent=1) + '\n')
    print(f"{len(SHAPES)} listed shapes, {len(shapes)} behind each digest, {len(SETTINGS)} settings, {len(table['fuzz_cases'])} fuzz cases")


if __name__ == '__main__':
    main()
