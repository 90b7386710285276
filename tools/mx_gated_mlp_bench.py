"""MXGatedMLP (fewbit_amd/glu.py, fewbit_amd/csrc/fewbit_mxglu.hip) on MI355X at 16384 tokens, 4096 -> 11008 and 768 -> 3072, bf16 and fp16.
Arms per case, alternating in one process:
  the layer forward + backward (torch.autograd.grad of the input and the three weights on a random gradient):
    fewbit.MXGatedMLP('fp4'), fewbit.MXGatedMLP('fp6'), fewbit.QuantizedGatedMLP(fused=True, bits=4), the torch MLP (three nn.Linear, F.silu);
  each new kernel alone against its byte floor at 8 TB/s, into preallocated outputs: cabi_x.mx_glu_forward (reads gate and up, writes y and the state)
  and cabi_x.mx_glu_backward (reads gy and the state, writes d_gate, d_up and three cell buffers), at fp4 and fp6.
Timing as tools/sketch_bench.py::timed (HIP events around many back-to-back calls after the GPU has settled, median over rounds); the arms alternate
twice and the smaller median is quoted.  Beside the times: bytes saved for backward per token (fewbit.memory_usage_hooks, the weights taken off), the
allocator's peak over one backward, and the relative error of each weight gradient of the same run against a float64 MLP on the same values.

    python tools/mx_gated_mlp_bench.py [--out FILE]        ->  profiles/mx_gated_mlp_bench.json
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
CASES = tuple((hidden, inter, dtype) for hidden, inter in ((4096, 11008), (768, 3072)) for dtype in (torch.bfloat16, torch.float16))
FORMATS = ('fp4', 'fp6')
PEAK_BYTES_PER_US = 8.0e6


class TorchMLP(torch.nn.Module):
    def __init__(self, hidden, inter, dtype):
        super().__init__()
        self.gate_proj, self.up_proj = (torch.nn.Linear(hidden, inter, False, DEV, dtype) for _ in range(2))
        self.down_proj, self.act_fn = torch.nn.Linear(inter, hidden, False, DEV, dtype), torch.nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


def weights_of(m):
    return m.gate_proj.weight, m.up_proj.weight, m.down_proj.weight


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
    torch.autograd.grad(y, (x, *weights_of(m)), gy)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mx_gated_mlp_bench.json'), help='where the record is written')
    ap.add_argument('--reps', type=int, default=10, help='back-to-back calls per timed round')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    rows = []
    for hidden, inter, dtype in CASES:
        torch.manual_seed(0)
        base = TorchMLP(hidden, inter, dtype)
        x = torch.randn(TOKENS, hidden, device=DEV).to(dtype).requires_grad_()
        gy = torch.randn(TOKENS, hidden, device=DEV).to(dtype)
        layers = {'torch_mlp': base, 'quantized_fused_4': fewbit.QuantizedGatedMLP.from_mlp(base, bits=4, fused=True)}
        for fmt in FORMATS:
            layers[f'mx_{fmt}'] = fewbit.MXGatedMLP.from_mlp(base, format=fmt)                # one set of parameters
        step = lambda m: torch.autograd.grad(m(x), (x, *weights_of(m)), gy)
        arms = {f'layer_{name}': (lambda m=m: step(m), args.reps) for name, m in layers.items()}
        # the kernels alone
        gate, up = (torch.randn(TOKENS, inter, device=DEV).to(dtype) for _ in range(2))
        both, y = torch.empty(TOKENS, 2 * inter, device=DEV, dtype=dtype), torch.empty(TOKENS, inter, device=DEV, dtype=dtype)
        states = {fmt: cabi_x.mx_glu_forward(gate, up, 'silu', fmt, SEEDS[:2])[1] for fmt in FORMATS}
        for fmt in FORMATS:
            arms[f'mx_glu_forward_{fmt}'] = (lambda fmt=fmt: cabi_x.mx_glu_forward(gate, up, 'silu', fmt, SEEDS[:2], y=y, state=states[fmt]), 2 * args.reps)
            arms[f'mx_glu_backward_{fmt}'] = (lambda fmt=fmt: cabi_x.mx_glu_backward(y, states[fmt], 'silu', fmt, SEEDS[2:], d_gate=both[:, :inter], d_up=both[:, inter:]),
                                              2 * args.reps)
        runs = {name: [] for name in arms}
        for f, _ in arms.values():                                   # every arm once before any is timed: allocator, code objects, clocks
            timed(f, reps=3, rounds=1)
        for _ in range(2):
            for name, (f, reps) in arms.items():
                runs[name].append(round(timed(f, reps=reps), 2))
        us = {name: min(v) for name, v in runs.items()}
        # the errors of one run against float64 on the same values, a chunk of the tokens at a time
        x64, w64 = x.detach().double(), [w.detach().double().requires_grad_() for w in weights_of(base)]
        exact = [torch.zeros_like(w) for w in w64]
        for at in range(0, TOKENS, 2048):
            part = F.linear(F.silu(F.linear(x64[at:at + 2048], w64[0])) * F.linear(x64[at:at + 2048], w64[1]), w64[2])
            for total, g in zip(exact, torch.autograd.grad(part, w64, gy[at:at + 2048].double())):
                total += g
        error = {name: {w: round(float((g.double() - e).norm() / e.norm()), 5) for w, g, e in zip(('gate', 'up', 'down'), step(m)[1:], exact)} for name, m in layers.items()}
        del x64, w64, exact
        size, weights = x.element_size(), sum(w.numel() for w in weights_of(base)) * x.element_size()
        kernels = {}
        for fmt in FORMATS:
            cells, grads = cabi_x.mx_bytes(TOKENS, inter, fmt), cabi_x.mx_bytes(TOKENS, inter, 'fp8')
            for name, moved in ((f'mx_glu_forward_{fmt}', 3 * size * gate.numel() + 2 * cells), (f'mx_glu_backward_{fmt}', 3 * size * gate.numel() + 3 * cells + 2 * grads)):
                floor = moved / PEAK_BYTES_PER_US
                kernels[name] = {'bytes_moved': moved, 'byte_floor_us_at_8TBs': round(floor, 2), 'us': us[name], 'fraction_of_floor': round(floor / us[name], 3)}
        row = {'tokens': TOKENS, 'hidden': hidden, 'intermediate': inter, 'dtype': str(dtype).replace('torch.', ''), 'us': us, 'runs_us': runs,
               'layer_over_torch_mlp': {name: round(us[f'layer_{name}'] / us['layer_torch_mlp'], 4) for name in layers},
               'layer_over_quantized_fused_4': {name: round(us[f'layer_{name}'] / us['layer_quantized_fused_4'], 4) for name in layers},
               'saved_for_backward_bytes_per_token': {name: round((saved_bytes(lambda m=m: m(x)) - weights) / TOKENS, 1) for name, m in layers.items()},
               'backward_peak_bytes': {name: backward_peak(m, x, gy) for name, m in layers.items()},
               'weight_gradient_relative_error_of_one_call': error, 'kernels': kernels}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del arms, layers, base, x, gy, gate, up, both, y, states
        torch.cuda.empty_cache()
    record = {'what': 'python tools/mx_gated_mlp_bench.py: MXGatedMLP (fp4, fp6) forward + backward beside QuantizedGatedMLP(fused=True, bits=4) and the torch MLP, and '
                      'cabi_x.mx_glu_forward / mx_glu_backward alone against their byte floors; every arm in one process, alternating; us per call',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
