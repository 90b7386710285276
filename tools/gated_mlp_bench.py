"""The gated MLP as one node (fewbit_amd/glu.py, gated_mlp_quantized; fewbit_amd/csrc/fewbit_glu.hip, the PRODUCT kernels) on MI355X at 16384 tokens of
4096 -> 11008 (the MLP of Llama-7B) and 768 -> 3072, bf16 and fp32, 2 / 4 / 8 bits.  Arms per case, alternating in one process, each forward +
backward (torch.autograd.grad of x and the three weights on a random gradient):
  (a) down(F.silu(gate(x)) * up(x))                 three nn.Linear and torch's product: keeps x, gate, silu(gate), up and y;
  (b) fewbit.QuantizedGatedMLP(fused=False)         three nn.Linear around glu_quantized: keeps x, the state of gate and up, and y;
  (c) fewbit.QuantizedGatedMLP(fused=True)          ONE node: keeps x in a few bits, the state of gate and up, nothing of y;
and the new entry point alone, into preallocated outputs, for its share of the byte floor at 8 TB/s:
  (d) cabi_x.glu_backward_product                   floor: gy + state + d_gate + d_up + product bytes.
Timing as tools/sketch_bench.py::timed: the GPU is kept busy with the same call until it has settled, then the median over rounds of many
back-to-back calls between HIP events.  The arms alternate through FIVE invocations; quoted are the median of the five, and for (c) over (b) the
ratio of every invocation and its spread.  Bytes saved for backward are counted with torch.autograd.graph.saved_tensors_hooks, every storage once.
No time is fixed in advance: what is slower than the unfused module by more than the spread is listed as such.

    python tools/gated_mlp_bench.py [--out FILE]        ->  profiles/gated_mlp_bench.json
"""
import argparse
import json
import os
import statistics
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
TOKENS, SEED, INVOCATIONS = 16384, 2026, 5
CASES = tuple((width, hidden, dtype) for width, hidden in ((4096, 11008), (768, 3072)) for dtype in (torch.bfloat16, torch.float32))
BITS = (2, 4, 8)
PEAK_BYTES_PER_US = 8.0e6


def saved_bytes(f, parameters):
    """bytes of the storages autograd saved while `f` ran, each counted once (views of one tensor share it), those of `parameters` left out"""
    seen, own = {}, {p.untyped_storage().data_ptr() for p in parameters}

    def pack(t):
        seen[t.untyped_storage().data_ptr()] = t.untyped_storage().nbytes()
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        f()
    return sum(size for ptr, size in seen.items() if ptr not in own)


class Projections(torch.nn.Module):
    """the three projections of `mlp` under the names from_mlp looks for"""

    def __init__(self, mlp):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj, self.act_fn = mlp.gate_proj, mlp.up_proj, mlp.down_proj, torch.nn.SiLU()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gated_mlp_bench.json'), help='where the record is written')
    ap.add_argument('--reps', type=int, default=5, help='back-to-back calls per timed round')
    ap.add_argument('--tokens', type=int, default=TOKENS)
    ap.add_argument('--cases', default='', help='comma-separated indices into the list of cases (default: all)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    rows, slower = [], []
    chosen = [int(i) for i in args.cases.split(',')] if args.cases else range(len(CASES))
    for width, hidden, dtype in (CASES[i] for i in chosen):
        torch.manual_seed(0)
        mlp = fewbit.QuantizedGatedMLP(width, hidden, device=DEV, dtype=dtype)
        x = torch.randn(args.tokens, width, device=DEV).to(dtype).requires_grad_()
        g_out = torch.randn(args.tokens, width, device=DEV).to(dtype)
        leaves = (x, mlp.gate_proj.weight, mlp.up_proj.weight, mlp.down_proj.weight)
        modules = {'torch_mlp': lambda: mlp.down_proj(F.silu(mlp.gate_proj(x)) * mlp.up_proj(x))}
        for bits in BITS:
            for fused in (False, True):
                m = fewbit.QuantizedGatedMLP.from_mlp(Projections(mlp), bits=bits, fused=fused)
                modules[f'{"fused" if fused else "unfused"}_{bits}'] = lambda m=m: m(x)
        step = lambda forward: torch.autograd.grad(forward(), leaves, g_out)
        arms = {name: (lambda forward=forward: step(forward), args.reps) for name, forward in modules.items()}
        n, size = args.tokens * hidden, x.element_size()
        gy = torch.randn(args.tokens, hidden, device=DEV).to(dtype)
        gate, up = (1.5 * torch.randn(args.tokens, hidden, device=DEV)).to(dtype), (1.5 * torch.randn(args.tokens, hidden, device=DEV)).to(dtype)
        both, product = torch.empty(args.tokens, 2 * hidden, device=DEV, dtype=dtype), torch.empty(args.tokens, hidden, device=DEV, dtype=dtype)
        state = {bits: cabi_x.glu_forward(gate, up, 'silu', bits, SEED)[1] for bits in BITS}
        del gate, up
        for bits in BITS:
            arms[f'kernel_{bits}'] = (lambda bits=bits: cabi_x.glu_backward_product(gy, state[bits], 'silu', bits, (True, True, True), both[:, :hidden], both[:, hidden:], product),
                                      4 * args.reps)
        runs = {name: [] for name in arms}
        for f, _ in arms.values():                                   # every arm once before any is timed: allocator, code objects, library plans, clocks
            timed(f, reps=3, rounds=1)
        for _ in range(INVOCATIONS):
            for name, (f, reps) in arms.items():
                runs[name].append(round(timed(f, reps=reps), 2))
        us = {name: statistics.median(v) for name, v in runs.items()}
        kernels, ratios = {}, {}
        for bits in BITS:
            moved = 4 * size * n + cabi_x.glu_state_bytes(n, bits)   # gy + d_gate + d_up + product + state
            floor = moved / PEAK_BYTES_PER_US
            kernels[str(bits)] = {'bytes_moved': moved, 'byte_floor_us_at_8TBs': round(floor, 2), 'us': us[f'kernel_{bits}'], 'runs_us': runs[f'kernel_{bits}'],
                                  'fraction_of_floor': round(floor / us[f'kernel_{bits}'], 3)}
            each = [round(f / u, 4) for f, u in zip(runs[f'fused_{bits}'], runs[f'unfused_{bits}'])]
            # the spread of the same arm over the invocations, relative: what a ratio has to exceed to mean anything
            noise = max((max(runs[name]) - min(runs[name])) / us[name] for name in (f'fused_{bits}', f'unfused_{bits}'))
            ratios[str(bits)] = {'fused_over_unfused': round(us[f'fused_{bits}'] / us[f'unfused_{bits}'], 4), 'of_every_invocation': each,
                                 'spread_of_the_ratio': round(max(each) - min(each), 4), 'spread_of_one_arm': round(noise, 4),
                                 'fused_over_torch': round(us[f'fused_{bits}'] / us['torch_mlp'], 4)}
            if ratios[str(bits)]['fused_over_unfused'] - 1 > ratios[str(bits)]['spread_of_the_ratio']:
                slower.append(f'{width} -> {hidden} {dtype} bits {bits}: fused {us[f"fused_{bits}"]} us against {us[f"unfused_{bits}"]} us unfused')
        row = {'tokens': args.tokens, 'width': width, 'hidden': hidden, 'dtype': str(dtype).replace('torch.', ''),
               'us_forward_plus_backward': {name: us[name] for name in modules}, 'runs_us': {name: runs[name] for name in modules}, 'ratios': ratios,
               'saved_for_backward_bytes': {name: saved_bytes(forward, leaves[1:]) for name, forward in modules.items()},
               'saved_for_backward_bytes_per_token': {}, 'kernel_glu_backward_product': kernels}
        row['saved_for_backward_bytes_per_token'] = {name: round(v / args.tokens, 1) for name, v in row['saved_for_backward_bytes'].items()}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del arms, modules, mlp, x, g_out, gy, both, product, state, leaves
        torch.cuda.empty_cache()
    record = {'what': 'python tools/gated_mlp_bench.py: QuantizedGatedMLP(fused=True) forward + backward beside fused=False and the torch MLP, and the '
                      'glu_backward_product entry point alone; every arm in one process, alternating through five invocations; us per call (medians)',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'slower_than_unfused_beyond_the_spread': slower, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    print('slower than the unfused module beyond the spread:', slower or 'none')


if __name__ == '__main__':
    main()
