"""The dropout of a seed (fewbit_amd/dropout.py, fewbit_amd/csrc/fewbit_dropout.hip) on MI355X at the shapes of RoBERTa-base's hidden and
intermediate activations: 16384 x 768 and 16384 x 3072, bf16 and fp32, p = 0.1.  Arms per case, alternating in one process, each forward +
backward (torch.autograd.grad on a random gradient):
  (a) fewbit.functional.dropout(x)                      one launch each way, nothing saved;
  (b) torch.nn.functional.dropout(x)                    torch's native dropout: one bool per element saved;
  (c) fewbit.functional.dropout_add(x, r)               the sum in the same launch;
  (d) r + torch.nn.functional.dropout(x)                what (c) replaces;
and the kernel alone, into a preallocated output, for its share of the byte floor:
  (e) cabi_x.dropout_apply(x, seed, p, out=out)         floor: 2 s n bytes (read x, write out) at 8 TB/s;
  (f) cabi_x.dropout_apply(x, seed, p, r, out=out)      floor: 3 s n bytes.
Timing as tools/sketch_bench.py::timed: the GPU is kept busy with the same call until it has settled, then the median over rounds of many
back-to-back calls between HIP events; the arms alternate twice and the smaller median is quoted.  Bytes saved for backward are counted with
fewbit.memory_usage_hooks.  The kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this script.

    python tools/dropout_bench.py [--out FILE]        ->  profiles/dropout_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # tools/ -> repository root
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch
import torch.nn.functional as F
import fewbit_amd as fewbit
from fewbit_amd import cabi_x
from sketch_bench import timed

DEV = 'cuda'
ROWS, P, SEED = 16384, 0.1, 2026
CASES = tuple((features, dtype) for features in (768, 3072) for dtype in (torch.bfloat16, torch.float32))
PEAK_BYTES_PER_US = 8.0e6


def saved_bytes(f):
    with fewbit.memory_usage_hooks() as usage:
        f()
    return usage.forward or 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dropout_bench.json'), help='where the record is written')
    ap.add_argument('--reps', type=int, default=100, help='back-to-back calls per timed round')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    rows = []
    for features, dtype in CASES:
        x = torch.randn(ROWS, features, device=DEV).to(dtype).requires_grad_()
        r = torch.randn(ROWS, features, device=DEV).to(dtype).requires_grad_()
        gy = torch.randn(ROWS, features, device=DEV).to(dtype)
        xd, rd, out = x.detach(), r.detach(), torch.empty_like(gy)
        forward = {
            'fewbit_dropout': lambda: fewbit.functional.dropout(x, P),
            'torch_dropout': lambda: F.dropout(x, P),
            'fewbit_dropout_add': lambda: fewbit.functional.dropout_add(x, r, P),
            'torch_dropout_add': lambda: r + F.dropout(x, P),
        }
        arms = {name: (lambda f=f, wrt=(x, r) if name.endswith('_add') else (x, ): torch.autograd.grad(f(), wrt, gy), args.reps) for name, f in forward.items()}
        arms['kernel'] = (lambda: cabi_x.dropout_apply(xd, SEED, P, out=out), 2 * args.reps)
        arms['kernel_add'] = (lambda: cabi_x.dropout_apply(xd, SEED, P, rd, out=out), 2 * args.reps)
        runs = {name: [] for name in arms}
        for f, _ in arms.values():                                   # every arm once before any is timed: allocator, code objects, clocks
            timed(f, reps=10, rounds=1)
        for _ in range(2):
            for name, (f, reps) in arms.items():
                runs[name].append(round(timed(f, reps=reps), 2))
        us = {name: min(v) for name, v in runs.items()}
        n, size = ROWS * features, x.element_size()
        floor_us, floor_add_us = 2 * size * n / PEAK_BYTES_PER_US, 3 * size * n / PEAK_BYTES_PER_US
        row = {'rows': ROWS, 'features': features, 'dtype': str(dtype).replace('torch.', ''), 'p': P, 'threshold': cabi_x.dropout_threshold(P),
               'us_forward_plus_backward': {k: v for k, v in us.items() if not k.startswith('kernel')}, 'us_kernel': {k: v for k, v in us.items() if k.startswith('kernel')},
               'runs_us': runs,
               'fewbit_over_torch': round(us['fewbit_dropout'] / us['torch_dropout'], 4),
               'fewbit_add_over_torch_add': round(us['fewbit_dropout_add'] / us['torch_dropout_add'], 4),
               'saved_for_backward_bytes': {name: saved_bytes(f) for name, f in forward.items()},
               'kernel_byte_floor_us_at_8TBs': round(floor_us, 2), 'kernel_fraction_of_floor': round(floor_us / us['kernel'], 3),
               'kernel_add_byte_floor_us_at_8TBs': round(floor_add_us, 2), 'kernel_add_fraction_of_floor': round(floor_add_us / us['kernel_add'], 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del arms, forward, x, r, gy, xd, rd, out
        torch.cuda.empty_cache()
    record = {'what': 'python tools/dropout_bench.py: dropout and dropout_add forward + backward against torch, and the kernel alone; every arm in one '
                      'process, alternating; us per call',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'rows': rows,
              'verdict': {'fewbit_dropout_no_slower_than_torch_at_every_shape': all(r['fewbit_over_torch'] <= 1.0 for r in rows),
                          'fewbit_dropout_add_no_slower_than_torch_at_every_shape': all(r['fewbit_add_over_torch_add'] <= 1.0 for r in rows),
                          'fewbit_saves_nothing_for_backward': all(r['saved_for_backward_bytes']['fewbit_dropout'] == 0 and r['saved_for_backward_bytes']['fewbit_dropout_add'] == 0
                                                                   for r in rows)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    print(json.dumps(record['verdict']))


if __name__ == '__main__':
    main()
