"""MXLayerNormLinear (fewbit_amd/norm.py, fewbit_amd/csrc/fewbit_mxlnorm.hip) on MI355X at 16384 tokens, bf16 and fp16, at 768 -> 3 x 768 (RoBERTa-base
q / k / v), 768 -> 3072 with return_normed=True (its intermediate dense: y also feeds the next residual, and takes a gradient of its own) and
4096 -> (4096, 1024, 1024) (beside EXPERIMENTS 8.34).  Every linear has a bias.  Arms per case, alternating in one process:
  the norm and its linears forward + backward (torch.autograd.grad of the input, the norm's weight and bias and every weight and bias on random gradients):
    fewbit.MXLayerNormLinear('fp4'), ('fp6'), fewbit.QuantizedLayerNorm(bits=4) + k fewbit.MXLinear('fp4'), torch LayerNorm + k nn.Linear;
  each new kernel alone against its byte floor at 8 TB/s, into preallocated outputs, beside what it replaces on the same tensors:
    cabi_x.mx_layer_norm_forward (reads x, writes y, mean, rstd and the cells) beside cabi_x.layer_norm_forward(bits=4) + one cabi_x.mx_pack of its y,
    cabi_x.mx_layer_norm_backward (reads gy and the cells, writes dx, dgamma and dbeta) beside cabi_x.layer_norm_backward(bits=4).
Timing as tools/sketch_bench.py::timed (HIP events around many back-to-back calls after the GPU has settled, median over rounds); the arms alternate
twice and the smaller median is quoted.  Beside the times: bytes saved for backward per token (fewbit.memory_usage_hooks, the parameters taken off)
next to the derived mx_bytes / rows + 4, and the allocator's peak over one backward.

    python tools/mx_layer_norm_linear_bench.py [--out FILE]        ->  profiles/mx_layer_norm_linear_bench.json
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
TOKENS, SEED, EPS = 16384, 2026, 1e-5
SHAPES = ((768, (768, 768, 768), False), (768, (3072, ), True), (4096, (4096, 1024, 1024), False))       # width, the linears, return_normed
CASES = tuple((*shape, dtype) for shape in SHAPES for dtype in (torch.bfloat16, torch.float16))
FORMATS = ('fp4', 'fp6')
PEAK_BYTES_PER_US = 8.0e6


class Composed(torch.nn.Module):
    """a norm module and the linears that read it, as separate nodes"""

    def __init__(self, norm, linears, return_normed):
        super().__init__()
        self.norm, self.linears, self.return_normed = norm, torch.nn.ModuleList(linears), return_normed

    def forward(self, x):
        y = self.norm(x)
        outs = tuple(m(y) for m in self.linears)
        return (y, *outs) if self.return_normed else outs


def parameters_of(m):
    norm = m if isinstance(m, fewbit.MXLayerNormLinear) else m.norm
    return (norm.weight, norm.bias, *(lin.weight for lin in m.linears), *(lin.bias for lin in m.linears))


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mx_layer_norm_linear_bench.json'), help='where the record is written')
    ap.add_argument('--reps', type=int, default=10, help='back-to-back calls per timed round')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    rows = []
    for width, outs, normed, dtype in CASES:
        torch.manual_seed(0)
        norm = torch.nn.LayerNorm(width, EPS, device=DEV, dtype=dtype)
        with torch.no_grad():
            norm.bias.normal_()
        linears = [torch.nn.Linear(width, n, True, DEV, dtype) for n in outs]
        x = torch.randn(TOKENS, width, device=DEV).to(dtype).requires_grad_()
        grads = [torch.randn(TOKENS, n, device=DEV).to(dtype) for n in ((width, ) if normed else ()) + outs]
        layers = {'torch': Composed(norm, linears, normed),                                        # one set of parameters
                  'quantized_4_mx_linear': Composed(fewbit.QuantizedLayerNorm.from_layer_norm(norm, bits=4), [fewbit.MXLinear.from_linear(m, 'fp4') for m in linears],
                                                    normed)}
        for fmt in FORMATS:
            layers[f'mx_layer_norm_linear_{fmt}'] = fewbit.MXLayerNormLinear.from_modules(norm, linears, format=fmt, return_normed=normed)
        step = lambda m: torch.autograd.grad(m(x), (x, *parameters_of(m)), grads)
        arms = {f'layer_{name}': (lambda m=m: step(m), args.reps) for name, m in layers.items()}
        # the kernels alone, beside what they replace
        xd, gamma, beta, gy = x.detach(), norm.weight.detach(), norm.bias.detach(), torch.randn(TOKENS, width, device=DEV).to(dtype)
        y, out = torch.empty_like(xd), torch.empty_like(xd)
        mean, rstd, dgamma, dbeta = torch.empty(TOKENS, device=DEV), torch.empty(TOKENS, device=DEV), torch.empty(width, device=DEV), torch.empty(width, device=DEV)
        cells = {fmt: cabi_x.mx_layer_norm_forward(xd, gamma, beta, EPS, fmt, SEED)[1] for fmt in FORMATS}
        state = cabi_x.layer_norm_forward(xd, gamma, beta, EPS, 4, SEED)[2]
        packed = torch.empty(cabi_x.mx_bytes(TOKENS, width, 'fp4'), dtype=torch.uint8, device=DEV)
        spaces = (torch.empty(cabi_x.mx_layer_norm_workspace(TOKENS, width), dtype=torch.uint8, device=DEV),
                  torch.empty(cabi_x.norm_workspace_bytes(TOKENS, width), dtype=torch.uint8, device=DEV))
        for fmt in FORMATS:
            arms[f'mx_layer_norm_forward_{fmt}'] = (lambda fmt=fmt: cabi_x.mx_layer_norm_forward(xd, gamma, beta, EPS, fmt, SEED, y=y, mean=mean, rstd=rstd,
                                                                                                 cells=cells[fmt]), 2 * args.reps)
            arms[f'mx_layer_norm_backward_{fmt}'] = (lambda fmt=fmt: cabi_x.mx_layer_norm_backward(gy, cells[fmt], rstd, gamma, fmt, dx=out, dgamma=dgamma, dbeta=dbeta,
                                                                                                   workspace=spaces[0]), 2 * args.reps)
        arms['layer_norm_forward_4_then_mx_pack_fp4'] = (lambda: (cabi_x.layer_norm_forward(xd, gamma, beta, EPS, 4, SEED, y=y, rstd=rstd, state=state),
                                                                  cabi_x.mx_pack(y, SEED + 1, 'fp4', out=packed)), 2 * args.reps)
        arms['layer_norm_backward_4'] = (lambda: cabi_x.layer_norm_backward(gy, state, rstd, gamma, 4, dx=out, dgamma=dgamma, dbeta=dbeta, workspace=spaces[1]),
                                         2 * args.reps)
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
            for name, old in ((f'mx_layer_norm_forward_{fmt}', 'layer_norm_forward_4_then_mx_pack_fp4'), (f'mx_layer_norm_backward_{fmt}', 'layer_norm_backward_4')):
                floor = moved / PEAK_BYTES_PER_US
                kernels[name] = {'bytes_moved': moved, 'byte_floor_us_at_8TBs': round(floor, 2), 'us': us[name], 'fraction_of_floor': round(floor / us[name], 3),
                                 'beside': old, 'beside_us': us[old], 'over_beside': round(us[name] / us[old], 4)}
        row = {'tokens': TOKENS, 'width': width, 'outs': list(outs), 'return_normed': normed, 'dtype': str(dtype).replace('torch.', ''), 'us': us, 'runs_us': runs,
               'layer_over_torch': {name: round(us[f'layer_{name}'] / us['layer_torch'], 4) for name in layers},
               'layer_over_quantized_4_mx_linear': {name: round(us[f'layer_{name}'] / us['layer_quantized_4_mx_linear'], 4) for name in layers},
               'saved_for_backward_bytes_per_token': {name: round((saved_bytes(lambda m=m: m(x)) - parameters) / TOKENS, 1) for name, m in layers.items()},
               'derived_bytes_per_token': {fmt: cabi_x.mx_bytes(TOKENS, width, fmt) / TOKENS + 4 for fmt in FORMATS},
               'backward_peak_bytes': {name: backward_peak(m, x, grads) for name, m in layers.items()}, 'kernels': kernels}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del arms, layers, norm, linears, x, grads, xd, gy, y, out, cells, state, packed, spaces
        torch.cuda.empty_cache()
    record = {'what': 'python tools/mx_layer_norm_linear_bench.py: MXLayerNormLinear (fp4, fp6) forward + backward beside QuantizedLayerNorm(bits=4) + k MXLinear '
                      'and torch LayerNorm + k nn.Linear, and cabi_x.mx_layer_norm_forward / mx_layer_norm_backward alone against their byte floors and beside '
                      'layer_norm_forward + mx_pack / layer_norm_backward; every arm in one process, alternating; us per call',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
