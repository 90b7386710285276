#!/usr/bin/env python3
"""Every plan the activation unit of libfewbit_hip.so makes, as fewbit_hip_describe_* prints it: the sibling of tools/core_refusal_digest.py for the calls
that are NOT refused.  Nothing is launched: the tool calls only the four describe entry points (and fewbit_hip_tune) through fewbit_amd.cabi's library
handle, one line per call with the arguments and the JSON returned.  Two trees whose listings agree on one machine pick the same kernel instantiation
and the same launch shape for every call of the sweep: how a clean-up of the dispatch and launch code is shown to change no plan.  The listing depends
on the device's CU count and on the runtime's occupancy answers, so it is compared between two trees in one visit, not against a committed file.

    python tools/plan_digest.py [--root TREE] [--digest FILE] > listing.txt       # needs the GPU; --root: the tree whose package and library are asked

The sweep: every continuous functor x the three dtypes x 1, 2, 3, 4, 7, 8, 15, 16, 31 and 255 borders; the backward with 2, 3, 4, 8, 16, 17 and 256
levels; every stepwise functor, both directions; each at n = 1, 511, 512, 513 and one tile below, at and one tile above every threshold of the policy
code (4 Mi, 4.5 Mi, 6 Mi, 12 Mi, 20 Mi and 32 Mi elements, and the resident / chunked boundaries of launch_shape for this device's CU count: the
resident tile count and `ratio` times it, for each class of kernel, each number of resident blocks per CU that occurs and one and two groups per
lane); and all of that again with each of the eight tune keys at -1, 0, 1, 2, 3 and 4 in turn (restored to -1 afterwards).  The listing is some
hundred MB, so `--digest FILE` also writes what is small enough to keep: per entry point and tune setting the number of lines and their sha256.
"""
import argparse
import ctypes
import hashlib
import os
import sys

ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--digest', default=None)
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from fewbit_amd import cabi  # noqa: E402

MI = 1 << 20
KEYS = ('waves_per_cu', 'chunk', 'lut_chunk', 'lut_blocks_per_cu', 'lut_min', 'u_fwd', 'u_bwd', 'u_step1')
BORDERS, LEVELS = (1, 2, 3, 4, 7, 8, 15, 16, 31, 255), (2, 3, 4, 8, 16, 17, 256)
DTYPES = (0, 1, 2)


def counts(cus):
    ns = {1, 511, 512, 513}
    edges = [(t, 512) for t in (4 * MI, 9 * MI // 2, 6 * MI, 12 * MI, 20 * MI, 32 * MI)]
    # (waves per block, resident blocks per CU, ratio of the chunked shape): the table class, then the 256-thread class at 8, 6 and 4 blocks per CU
    for wpb, per_cu, ratio in ((16, 2, 12), (16, 1, 12), (4, 8, 4), (4, 6, 4), (4, 4, 4)):
        for u in (1, 2):
            resident = cus * per_cu * wpb * u * 512
            edges += [(resident, u * 512), (ratio * resident, u * 512)]
    for at, tile in edges:
        ns.update((at - tile, at, at + tile))
    return sorted(ns)


def main():
    assert torch.cuda.is_available(), 'the plans are those of a device'
    torch.cuda.set_device(0)
    torch.zeros(1, device='cuda')                                   # (the context: the describe calls ask for the current device)
    lib = cabi.lib()
    ns = counts(torch.cuda.get_device_properties(0).multi_processor_count)
    buf = ctypes.create_string_buffer(512)
    out, sections = sys.stdout, []

    def sweep(setting):
        def section(name, calls):
            h, lines = hashlib.sha256(), 0
            for call_args in calls:
                rc = getattr(lib, 'fewbit_hip_describe_' + name)(*call_args, buf, len(buf))
                line = f'{setting} {name}{call_args} -> {buf.value.decode() if rc == 0 else (rc, lib.fewbit_hip_last_error().decode())}\n'
                out.write(line)
                h.update(line.encode())
                lines += 1
            sections.append(f'{setting} {name}: {lines} lines, sha256 {h.hexdigest()}')
        section('quantize_forward', ((fn, dt, n, nb) for fn in range(len(cabi.CONTINUOUS)) for dt in DTYPES for nb in BORDERS for n in ns))
        section('quantize_backward', ((dt, n, nl) for dt in DTYPES for nl in LEVELS for n in ns))
        section('stepwise1_forward', ((fn, dt, n) for fn in range(len(cabi.STEPWISE1)) for dt in DTYPES for n in ns))
        section('stepwise1_backward', ((fn, dt, n) for fn in range(len(cabi.STEPWISE1)) for dt in DTYPES for n in ns))

    sweep('policy')
    for key in KEYS:
        for value in (-1, 0, 1, 2, 3, 4):
            cabi.tune(**{key: value})
            try:
                sweep(f'{key}={value}')
            finally:
                cabi.tune(**{key: -1})
    # the describe calls' own refusal, which needs a device to get as far: no buffer, no length
    for what, b, length in (('buf=NULL', None, 512), ('len=0', buf, 0)):
        rc = lib.fewbit_hip_describe_quantize_forward(2, 2, 8, 15, b, length)
        line = f'policy quantize_forward [{what}] -> {rc} "{lib.fewbit_hip_last_error().decode()}"'
        out.write(line + '\n')
        sections.append(line)
    if args.digest:
        with open(args.digest, 'w') as f:
            f.write(f'# tools/plan_digest.py: {len(ns)} element counts, {torch.cuda.get_device_properties(0).multi_processor_count} CUs\n' + '\n'.join(sections) + '\n')


if __name__ == '__main__':
    main()
