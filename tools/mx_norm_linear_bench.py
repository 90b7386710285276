"""MXNormLinear (fewbit_amd/norm.py, fewbit_amd/csrc/fewbit_mxnorm.hip) on MI355X at 16384 tokens, 4096 -> (4096, 1024, 1024) and 768 -> (768, 768, 768),
bf16 and fp16.  Arms per case, alternating in one process:
  the norm and its three linears forward + backward (torch.autograd.grad of the input, the norm's weight and the three weights on random gradients):
    fewbit.MXNormLinear('fp4'), fewbit.MXNormLinear('fp6'), fewbit.QuantizedRMSNorm(bits=4) + three fewbit.MXLinear('fp4'), torch RMSNorm + three nn.Linear;
  each new kernel alone against its byte floor at 8 TB/s, into preallocated outputs, beside what it replaces on the same tensors:
    cabi_x.mx_rms_norm_forward (reads x, writes y, rstd and the cells) beside cabi_x.rms_norm_forward(bits=4) + one cabi_x.mx_pack of its y,
    cabi_x.mx_rms_norm_backward (reads gy and the cells, writes dx and dgamma) beside cabi_x.rms_norm_backward(bits=4).
Timing as tools/sketch_bench.py::timed (HIP events around many back-to-back calls after the GPU has settled, median over rounds); the arms alternate
twice and the smaller median is quoted.  Beside the times: bytes saved for backward per token (fewbit.memory_usage_hooks, the parameters taken off)
next to the derived mx_bytes / rows + 4, and the allocator's peak over one backward.

    python tools/mx_norm_linear_bench.py [--out FILE]        ->  profiles/mx_norm_linear_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # tools/ -> repository root
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch
import fewbit_amd as fewbit
from fewbit_amd import cabi_x
from sketch_bench import timed

DEV = 'cuda'
TOKENS, SEED, EPS = 16384, 2026, 1e-6
CASES = tuple((width, outs, dtype) for width, outs in ((4096, (4096, 1024, 1024)), (768, (768, 768, 768))) for dtype in (torch.bfloat16, torch.float16))
FORMATS = ('fp4', 'fp6')
PEAK_BYTES_PER_US = 8.0e6


class Composed(torch.nn.Module):
    """a norm module and the linears that read it, as separate nodes"""

    def __init__(self, norm, linears):
        super().__init__()
        self.norm, self.linears = norm, torch.nn.ModuleList(linears)

    def forward(self, x):
        y = self.norm(x)
        return tuple(m(y) for m in self.linears)


def parameters_of(m):
    return (m.weight if isinstance(m, fewbit.MXNormLinear) else m.norm.weight, *(lin.weight for lin in m.linears))


def saved_bytes(f):
    with fewbit.memory_usage_hooks() as usage:
        f()
    return usage.forward or 0


def backward_peak(m, x, grads):
    """bytes by which the allocator's peak over ONE backward exceeds what was allocated before it"""
    outs = m(x)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    torch.autograd.grad(outs, (x, *parameters_of(m)), grads)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mx_norm_linear_bench.json'), help='where the record is written')
    ap.add_argument('--reps', type=int, default=10, help='back-to-back calls per timed round')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    rows = []
    for width, outs, dtype in CASES:
        torch.manual_seed(0)
        norm = torch.nn.RMSNorm(width, EPS, device=DEV, dtype=dtype)
        linears = [torch.nn.Linear(width, n, False, DEV, dtype) for n in outs]
        x = torch.randn(TOKENS, width, device=DEV).to(dtype).requires_grad_()
        grads = [torch.randn(TOKENS, n, device=DEV).to(dtype) for n in outs]
        layers = {'torch': Composed(norm, linears),                                                # one set of parameters
                  'quantized_4_mx_linear': Composed(fewbit.QuantizedRMSNorm.from_rms_norm(norm, bits=4), [fewbit.MXLinear.from_linear(m, 'fp4') for m in linears])}
        for fmt in FORMATS:
            layers[f'mx_norm_linear_{fmt}'] = fewbit.MXNormLinear.from_modules(norm, linears, format=fmt)
        step = lambda m: torch.autograd.grad(m(x), (x, *parameters_of(m)), grads)
        arms = {f'layer_{name}': (lambda m=m: step(m), args.reps) for name, m in layers.items()}
        # the kernels alone, beside what they replace
        xd, gamma, gy = x.detach(), norm.weight.detach(), torch.randn(TOKENS, width, device=DEV).to(dtype)
        y, out, rstd, dgamma = torch.empty_like(xd), torch.empty_like(xd), torch.empty(TOKENS, device=DEV), torch.empty(width, device=DEV)
        cells = {fmt: cabi_x.mx_rms_norm_forward(xd, gamma, EPS, fmt, SEED)[1] for fmt in FORMATS}
        state = cabi_x.rms_norm_forward(xd, gamma, EPS, 4, SEED)[2]
        packed = torch.empty(cabi_x.mx_bytes(TOKENS, width, 'fp4'), dtype=torch.uint8, device=DEV)
        spaces = (torch.empty(cabi_x.mx_rms_norm_workspace(TOKENS, width), dtype=torch.uint8, device=DEV),
                  torch.empty(cabi_x.norm_workspace_bytes(TOKENS, width), dtype=torch.uint8, device=DEV))
        for fmt in FORMATS:
            arms[f'mx_rms_norm_forward_{fmt}'] = (lambda fmt=fmt: cabi_x.mx_rms_norm_forward(xd, gamma, EPS, fmt, SEED, y=y, rstd=rstd, cells=cells[fmt]), 2 * args.reps)
            arms[f'mx_rms_norm_backward_{fmt}'] = (lambda fmt=fmt: cabi_x.mx_rms_norm_backward(gy, cells[fmt], rstd, gamma, fmt, dx=out, dgamma=dgamma,
                                                                                                workspace=spaces[0]), 2 * args.reps)
        arms['rms_norm_forward_4_then_mx_pack_fp4'] = (lambda: (cabi_x.rms_norm_forward(xd, gamma, EPS, 4, SEED, y=y, rstd=rstd, state=state),
                                                                cabi_x.mx_pack(y, SEED + 1, 'fp4', out=packed)), 2 * args.reps)
        arms['rms_norm_backward_4'] = (lambda: cabi_x.rms_norm_backward(gy, state, rstd, gamma, 4, dx=out, dgamma=dgamma, workspace=spaces[1]), 2 * args.reps)
        runs = {name: [] for name in arms}
        for f, _ in arms.values():                                   # every arm once before any is timed: allocator, code objects, clocks
            timed(f, reps=3, rounds=1)
        for _ in range(2):
            for name, (f, reps) in arms.items():
                runs[name].append(round(timed(f, reps=reps), 2))
        us = {name: min(v) for name, v in runs.items()}
        size = x.element_size()
        parameters = sum(p.numel() for p in parameters_of(layers['torch'])) * size
        kernels = {}
        for fmt in FORMATS:
            moved = 2 * size * x.numel() + cabi_x.mx_bytes(TOKENS, width, fmt) + 4 * TOKENS
            for name, old in ((f'mx_rms_norm_forward_{fmt}', 'rms_norm_forward_4_then_mx_pack_fp4'), (f'mx_rms_norm_backward_{fmt}', 'rms_norm_backward_4')):
                floor = moved / PEAK_BYTES_PER_US
                kernels[name] = {'bytes_moved': moved, 'byte_floor_us_at_8TBs': round(floor, 2), 'us': us[name], 'fraction_of_floor': round(floor / us[name], 3),
                                 'beside': old, 'beside_us': us[old], 'over_beside': round(us[name] / us[old], 4)}
        row = {'tokens': TOKENS, 'width': width, 'outs': list(outs), 'dtype': str(dtype).replace('torch.', ''), 'us': us, 'runs_us': runs,
               'layer_over_torch': {name: round(us[f'layer_{name}'] / us['layer_torch'], 4) for name in layers},
               'layer_over_quantized_4_mx_linear': {name: round(us[f'layer_{name}'] / us['layer_quantized_4_mx_linear'], 4) for name in layers},
               'saved_for_backward_bytes_per_token': {name: round((saved_bytes(lambda m=m: m(x)) - parameters) / TOKENS, 1) for name, m in layers.items()},
               'derived_bytes_per_token': {fmt: cabi_x.mx_bytes(TOKENS, width, fmt) / TOKENS + 4 for fmt in FORMATS},
               'backward_peak_bytes': {name: backward_peak(m, x, grads) for name, m in layers.items()}, 'kernels': kernels}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del arms, layers, norm, linears, x, grads, xd, gy, y, out, cells, state, packed, spaces
        torch.cuda.empty_cache()
    record = {'what': 'python tools/mx_norm_linear_bench.py: MXNormLinear (fp4, fp6) forward + backward beside QuantizedRMSNorm(bits=4) + three MXLinear and '
                      'torch RMSNorm + three nn.Linear, and cabi_x.mx_rms_norm_forward / mx_rms_norm_backward alone against their byte floors and beside '
                      'rms_norm_forward + mx_pack / rms_norm_backward; every arm in one process, alternating; us per call',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
