"""MXMLP (fewbit_amd/mlp.py, fewbit_amd/csrc/fewbit_mxact.hip) on MI355X at 16384 tokens, 768 -> 3072 -> 768 and 1024 -> 4096 -> 1024, bf16 and fp16, gelu.
Arms per case, alternating in one process:
  the layer forward + backward (torch.autograd.grad of the input, both weights and both biases on a random gradient):
    fewbit.MXMLP('fp4'), fewbit.MXMLP('fp6'), MXLinear -> fewbit.GELU(bits=3) -> MXLinear at each format (today's composition), the torch MLP;
  each new kernel alone against its byte floor at 8 TB/s, into preallocated outputs: cabi_x.mx_act_forward (reads u, writes h and one cell buffer) and
  cabi_x.mx_act_backward (reads gh and the cells, writes du and two cell buffers);
  the forward kernel beside what it replaces on the same tensor, cabi_x.mx_pack + F.gelu;
  the backward kernel beside cabi_x.mx_glu_backward at the same width PER BYTE MOVED: the column pair in a lane against the 32 x 64 tile through LDS.
Timing as tools/sketch_bench.py::timed (HIP events around many back-to-back calls after the GPU has settled, median over rounds); the arms alternate
twice and the smaller median is quoted.  Beside the times: bytes saved for backward per token (fewbit.memory_usage_hooks, the weights taken off) and
the allocator's peak over one backward.

    python tools/mx_mlp_bench.py [--out FILE]        ->  profiles/mx_mlp_bench.json
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
TOKENS, SEEDS = 16384, (2026, 2027, 2028, 2029, 2030)
CASES = tuple((hidden, inter, dtype) for hidden, inter in ((768, 3072), (1024, 4096)) for dtype in (torch.bfloat16, torch.float16))
FORMATS = ('fp4', 'fp6')
PEAK_BYTES_PER_US = 8.0e6


def saved_bytes(f):
    with fewbit.memory_usage_hooks() as usage:
        f()
    return usage.forward or 0


def backward_peak(m, x, gy):
    """bytes by which the allocator's peak over ONE backward exceeds what was allocated before it"""
    y = m(x)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    torch.autograd.grad(y, (x, *m.parameters()), gy)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mx_mlp_bench.json'), help='where the record is written')
    ap.add_argument('--reps', type=int, default=10, help='back-to-back calls per timed round')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    rows = []
    for hidden, inter, dtype in CASES:
        torch.manual_seed(0)
        fc1, fc2 = torch.nn.Linear(hidden, inter, True, DEV, dtype), torch.nn.Linear(inter, hidden, True, DEV, dtype)
        x = torch.randn(TOKENS, hidden, device=DEV).to(dtype).requires_grad_()
        gy = torch.randn(TOKENS, hidden, device=DEV).to(dtype)
        layers = {'torch_mlp': torch.nn.Sequential(fc1, torch.nn.GELU(), fc2)}
        for fmt in FORMATS:                                               # one set of parameters
            layers[f'mx_{fmt}'] = fewbit.MXMLP.from_linears(fc1, fc2, 'gelu', fmt)
            layers[f'composed_{fmt}'] = torch.nn.Sequential(fewbit.MXLinear.from_linear(fc1, fmt), fewbit.GELU(bits=3), fewbit.MXLinear.from_linear(fc2, fmt))
        step = lambda m: torch.autograd.grad(m(x), (x, *m.parameters()), gy)
        arms = {f'layer_{name}': (lambda m=m: step(m), args.reps) for name, m in layers.items()}
        # the kernels alone
        u, gh = (torch.randn(TOKENS, inter, device=DEV).to(dtype) for _ in range(2))
        h, du, both = torch.empty_like(u), torch.empty_like(u), torch.empty(TOKENS, 2 * inter, device=DEV, dtype=dtype)
        states = {fmt: cabi_x.mx_act_forward(u, 'gelu', fmt, SEEDS[0])[1] for fmt in FORMATS}
        glu_states = {fmt: cabi_x.mx_glu_forward(u, gh, 'gelu', fmt, SEEDS[:2])[1] for fmt in FORMATS}
        cells = {fmt: (torch.empty(cabi_x.mx_bytes(TOKENS, inter, 'fp8'), dtype=torch.uint8, device=DEV), torch.empty(cabi_x.mx_bytes(TOKENS, inter, fmt), dtype=torch.uint8, device=DEV))
                 for fmt in FORMATS}
        for fmt in FORMATS:
            arms[f'mx_act_forward_{fmt}'] = (lambda fmt=fmt: cabi_x.mx_act_forward(u, 'gelu', fmt, SEEDS[0], h=h, state=states[fmt]), 2 * args.reps)
            arms[f'mx_pack_plus_gelu_{fmt}'] = (lambda fmt=fmt: (cabi_x.mx_pack(u, SEEDS[0], fmt, 'kept', out=states[fmt]), F.gelu(u)), 2 * args.reps)
            arms[f'mx_act_backward_{fmt}'] = (lambda fmt=fmt: cabi_x.mx_act_backward(gh, states[fmt], 'gelu', fmt, SEEDS[1:3], (True, True, True), du, *cells[fmt]), 2 * args.reps)
            arms[f'mx_glu_backward_{fmt}'] = (lambda fmt=fmt: cabi_x.mx_glu_backward(gh, glu_states[fmt], 'gelu', fmt, SEEDS[2:], d_gate=both[:, :inter], d_up=both[:, inter:]),
                                              2 * args.reps)
        runs = {name: [] for name in arms}
        for f, _ in arms.values():                                   # every arm once before any is timed: allocator, code objects, clocks
            timed(f, reps=3, rounds=1)
        for _ in range(2):
            for name, (f, reps) in arms.items():
                runs[name].append(round(timed(f, reps=reps), 2))
        us = {name: min(v) for name, v in runs.items()}
        size, weights = x.element_size(), sum(p.numel() for p in (*fc1.parameters(), *fc2.parameters())) * x.element_size()
        kernels = {}
        for fmt in FORMATS:
            kept, grads, n = cabi_x.mx_bytes(TOKENS, inter, fmt), cabi_x.mx_bytes(TOKENS, inter, 'fp8'), u.numel()
            for name, moved in ((f'mx_act_forward_{fmt}', 2 * size * n + kept), (f'mx_pack_plus_gelu_{fmt}', 3 * size * n + kept),
                                (f'mx_act_backward_{fmt}', 2 * size * n + 2 * kept + grads), (f'mx_glu_backward_{fmt}', 3 * size * n + 3 * kept + 2 * grads)):
                floor = moved / PEAK_BYTES_PER_US
                kernels[name] = {'bytes_moved': moved, 'byte_floor_us_at_8TBs': round(floor, 2), 'us': us[name], 'fraction_of_floor': round(floor / us[name], 3)}
            kernels[f'forward_over_pack_plus_gelu_{fmt}'] = round(us[f'mx_act_forward_{fmt}'] / us[f'mx_pack_plus_gelu_{fmt}'], 4)
            # the two walks per byte moved: above 1, the column pair in a lane is the slower walk
            kernels[f'pair_walk_over_tile_walk_per_byte_{fmt}'] = round(kernels[f'mx_glu_backward_{fmt}']['fraction_of_floor'] / kernels[f'mx_act_backward_{fmt}']['fraction_of_floor'], 4)
        row = {'tokens': TOKENS, 'hidden': hidden, 'intermediate': inter, 'dtype': str(dtype).replace('torch.', ''), 'activation': 'gelu', 'us': us, 'runs_us': runs,
               'layer_over_torch_mlp': {name: round(us[f'layer_{name}'] / us['layer_torch_mlp'], 4) for name in layers},
               'mx_over_composed': {fmt: round(us[f'layer_mx_{fmt}'] / us[f'layer_composed_{fmt}'], 4) for fmt in FORMATS},
               'saved_for_backward_bytes_per_token': {name: round((saved_bytes(lambda m=m: m(x)) - weights) / TOKENS, 1) for name, m in layers.items()},
               'backward_peak_bytes': {name: backward_peak(m, x, gy) for name, m in layers.items()}, 'kernels': kernels}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del arms, layers, fc1, fc2, x, gy, u, gh, h, du, both, states, glu_states, cells
        torch.cuda.empty_cache()
    record = {'what': 'python tools/mx_mlp_bench.py: MXMLP (fp4, fp6) forward + backward beside MXLinear -> GELU(bits=3) -> MXLinear and the torch MLP; '
                      'cabi_x.mx_act_forward / mx_act_backward alone against their byte floors, the forward beside mx_pack + F.gelu, the backward beside '
                      'mx_glu_backward per byte moved (the two walks); every arm in one process, alternating; us per call',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
