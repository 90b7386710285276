"""glu_quantized (fewbit_amd/glu.py, fewbit_amd/csrc/fewbit_glu.hip) on MI355X at 16384 rows of 3072 and 11008 elements (the intermediate width of
Llama-7B), bf16 and fp32.  Arms per case, alternating in one process, each forward + backward (torch.autograd.grad of gate and up on a random
gradient):
  (a) F.silu(gate) * up                                             keeps gate, silu(gate) and up;
  (b) fewbit.functional.glu_quantized(gate, up, 'silu', 2 / 4 / 8)  keeps both inputs in a few bits;
and the entry points alone, into preallocated outputs, for their share of the byte floor at 8 TB/s:
  (c) cabi_x.glu_forward                                            floor: gate + up + y + state bytes;
  (d) cabi_x.glu_backward                                           floor: gy + state + d_gate + d_up bytes;
  (e) cabi_x.glu_forward(keep=False)                                the plain forward: gate + up + y bytes.
Timing as tools/sketch_bench.py::timed: the GPU is kept busy with the same call until it has settled, then the median over rounds of many
back-to-back calls between HIP events; the arms alternate twice and the smaller median is quoted.  Bytes saved for backward are counted with
fewbit.memory_usage_hooks.  Beside each quantized arm: the relative error of one gradient of gate and of up against float64.  No time is fixed in
advance: what is slower than torch is listed as such.

    python tools/glu_bench.py [--out FILE]        ->  profiles/glu_bench.json
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
ROWS, SEED = 16384, 2026
CASES = tuple((width, dtype) for width in (3072, 11008) for dtype in (torch.bfloat16, torch.float32))
BITS = (2, 4, 8)
PEAK_BYTES_PER_US = 8.0e6


def saved_bytes(f):
    with fewbit.memory_usage_hooks() as usage:
        f()
    return usage.forward or 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'glu_bench.json'), help='where the record is written')
    ap.add_argument('--reps', type=int, default=20, help='back-to-back calls per timed round')
    ap.add_argument('--rows', type=int, default=ROWS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    rows, slower = [], []
    for width, dtype in CASES:
        torch.manual_seed(0)
        gate = (1.5 * torch.randn(args.rows, width, device=DEV)).to(dtype).requires_grad_()
        up = (1.5 * torch.randn(args.rows, width, device=DEV)).to(dtype).requires_grad_()
        gy = torch.randn(args.rows, width, device=DEV).to(dtype)
        forwards = {'torch_silu_mul': lambda: F.silu(gate) * up}
        for bits in BITS:
            forwards[f'quantized_{bits}'] = lambda bits=bits: fewbit.functional.glu_quantized(gate, up, 'silu', bits)
        step = lambda forward: torch.autograd.grad(forward(), (gate, up), gy)
        arms = {name: (lambda forward=forward: step(forward), args.reps) for name, forward in forwards.items()}
        n, size, gd, ud = args.rows * width, gate.element_size(), gate.detach(), up.detach()
        y, d_gate, d_up = torch.empty_like(gd), torch.empty_like(gd), torch.empty_like(gd)
        state = {bits: cabi_x.glu_forward(gd, ud, 'silu', bits, SEED, y=y)[1] for bits in BITS}
        for bits in BITS:
            arms[f'forward_{bits}'] = (lambda bits=bits: cabi_x.glu_forward(gd, ud, 'silu', bits, SEED, y=y, state=state[bits]), 2 * args.reps)
            arms[f'backward_{bits}'] = (lambda bits=bits: cabi_x.glu_backward(gy, state[bits], 'silu', bits, d_gate=d_gate, d_up=d_up), 2 * args.reps)
        arms['forward_plain'] = (lambda: cabi_x.glu_forward(gd, ud, 'silu', keep=False, y=y), 2 * args.reps)
        runs = {name: [] for name in arms}
        for f, _ in arms.values():                                   # every arm once before any is timed: allocator, code objects, clocks
            timed(f, reps=5, rounds=1)
        for _ in range(2):
            for name, (f, reps) in arms.items():
                runs[name].append(round(timed(f, reps=reps), 2))
        us = {name: min(v) for name, v in runs.items()}
        g64, u64 = gd.double().requires_grad_(), ud.double().requires_grad_()
        exact = torch.autograd.grad(F.silu(g64) * u64, (g64, u64), gy.double())
        del g64, u64
        error = {}
        for name, forward in forwards.items():
            got = step(forward)
            error[name] = {'gate_gradient': round(float((got[0].double() - exact[0]).norm() / exact[0].norm()), 5),
                           'up_gradient': round(float((got[1].double() - exact[1]).norm() / exact[1].norm()), 5)}
            del got
        del exact
        kernels = {}
        for bits in BITS:
            kept = cabi_x.glu_state_bytes(n, bits)
            moved = 3 * size * n + kept                              # forward: gate + up + y + state; backward: gy + d_gate + d_up + state
            floor = moved / PEAK_BYTES_PER_US
            kernels[str(bits)] = {'bytes_moved': moved, 'byte_floor_us_at_8TBs': round(floor, 2), 'forward_us': us[f'forward_{bits}'], 'backward_us': us[f'backward_{bits}'],
                                  'forward_fraction_of_floor': round(floor / us[f'forward_{bits}'], 3),
                                  'backward_fraction_of_floor': round(floor / us[f'backward_{bits}'], 3)}
            if us[f'quantized_{bits}'] > us['torch_silu_mul']:
                slower.append(f'{width} {dtype} bits {bits}: {us[f"quantized_{bits}"]} us against {us["torch_silu_mul"]} us of F.silu(gate) * up')
        plain_floor = 3 * size * n / PEAK_BYTES_PER_US
        row = {'rows': args.rows, 'width': width, 'dtype': str(dtype).replace('torch.', ''),
               'us_forward_plus_backward': {name: us[name] for name in forwards}, 'runs_us': runs,
               'over_torch': {name: round(us[name] / us['torch_silu_mul'], 4) for name in forwards},
               'saved_for_backward_bytes': {name: saved_bytes(forward) for name, forward in forwards.items()},
               'input_bytes_gate_plus_up': 2 * size * n, 'kept_bytes': {str(bits): cabi_x.glu_state_bytes(n, bits) for bits in BITS},
               'plain_forward_us': us['forward_plain'], 'plain_forward_fraction_of_floor': round(plain_floor / us['forward_plain'], 3),
               'relative_error_of_one_call': error, 'kernels': kernels}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del arms, forwards, gate, up, gy, gd, ud, y, d_gate, d_up, state
        torch.cuda.empty_cache()
    record = {'what': "python tools/glu_bench.py: glu_quantized forward + backward beside F.silu(gate) * up, and the forward and backward entry points alone; "
                      'every arm in one process, alternating; us per call',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'slower_than_torch': slower, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    print('slower than torch:', slower or 'none')


if __name__ == '__main__':
    main()
