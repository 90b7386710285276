"""QuantizedLayerNorm (fewbit_amd/norm.py, fewbit_amd/csrc/fewbit_norm.hip) on MI355X at 16384 rows of RoBERTa-base's hidden size and of its MLP
width, 768 and 3072, bf16 and fp32.  Arms per case, alternating in one process, each forward + backward (torch.autograd.grad of the input,
gamma and beta on a random gradient):
  (a) torch.nn.LayerNorm                                            keeps its input, mean and rstd;
  (b) fewbit.QuantizedLayerNorm(bits=2 / 4 / 8)                     keeps the normalized rows in a few bits and rstd;
and the two entry points alone, into preallocated outputs, for their share of the byte floor at 8 TB/s:
  (c) cabi_x.layer_norm_forward                                     floor: x + y + state + rstd bytes;
  (d) cabi_x.layer_norm_backward (both launches)                    floor: gy + state + rstd + dx bytes.
Timing as tools/sketch_bench.py::timed: the GPU is kept busy with the same call until it has settled, then the median over rounds of many
back-to-back calls between HIP events; the arms alternate twice and the smaller median is quoted.  Bytes saved for backward are counted with
fewbit.memory_usage_hooks (gamma included, which every arm keeps).  Beside each quantized arm: the relative error of one input gradient and
of one gamma gradient against float64.

    python tools/layer_norm_bench.py [--out FILE]        ->  profiles/layer_norm_bench.json
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
ROWS, SEED, EPS = 16384, 2026, 1e-5
CASES = tuple((width, dtype) for width in (768, 3072) for dtype in (torch.bfloat16, torch.float32))
BITS = (2, 4, 8)
PEAK_BYTES_PER_US = 8.0e6


def saved_bytes(f):
    with fewbit.memory_usage_hooks() as usage:
        f()
    return usage.forward or 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'layer_norm_bench.json'), help='where the record is written')
    ap.add_argument('--reps', type=int, default=50, help='back-to-back calls per timed round')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    rows = []
    for width, dtype in CASES:
        torch.manual_seed(0)
        x = (3 + 2 * torch.randn(ROWS, width, device=DEV)).to(dtype).requires_grad_()
        gy = torch.randn(ROWS, width, device=DEV).to(dtype)
        layers = {'nn_layer_norm': torch.nn.LayerNorm(width, eps=EPS, device=DEV, dtype=dtype)}
        with torch.no_grad():
            layers['nn_layer_norm'].weight.copy_(1 + 0.5 * torch.randn(width, device=DEV))
            layers['nn_layer_norm'].bias.copy_(torch.randn(width, device=DEV))
        for bits in BITS:
            layers[f'quantized_{bits}'] = fewbit.QuantizedLayerNorm.from_layer_norm(layers['nn_layer_norm'], bits=bits)
        step = lambda layer: torch.autograd.grad(layer(x), (x, layer.weight, layer.bias), gy)
        arms = {name: (lambda layer=layer: step(layer), args.reps) for name, layer in layers.items()}
        n, size, xd = ROWS * width, x.element_size(), x.detach()
        gamma, beta = layers['nn_layer_norm'].weight.detach(), layers['nn_layer_norm'].bias.detach()
        y, dx, rstd = torch.empty_like(xd), torch.empty_like(xd), torch.empty(ROWS, dtype=torch.float32, device=DEV)
        dgamma, dbeta = torch.empty(width, dtype=torch.float32, device=DEV), torch.empty(width, dtype=torch.float32, device=DEV)
        workspace = torch.empty(cabi_x.norm_workspace_bytes(ROWS, width), dtype=torch.uint8, device=DEV)
        state = {bits: cabi_x.layer_norm_forward(xd, gamma, beta, EPS, bits, SEED, y=y, rstd=rstd)[2] for bits in BITS}
        for bits in BITS:
            arms[f'forward_{bits}'] = (lambda bits=bits: cabi_x.layer_norm_forward(xd, gamma, beta, EPS, bits, SEED, y=y, rstd=rstd, state=state[bits]), 2 * args.reps)
            arms[f'backward_{bits}'] = (lambda bits=bits: cabi_x.layer_norm_backward(gy, state[bits], rstd, gamma, bits, dx=dx, dgamma=dgamma, dbeta=dbeta,
                                                                                      workspace=workspace), 2 * args.reps)
        arms['forward_plain'] = (lambda: cabi_x.layer_norm_forward(xd, gamma, beta, EPS, keep=False, y=y, rstd=rstd), 2 * args.reps)
        runs = {name: [] for name in arms}
        for f, _ in arms.values():                                   # every arm once before any is timed: allocator, code objects, clocks
            timed(f, reps=10, rounds=1)
        for _ in range(2):
            for name, (f, reps) in arms.items():
                runs[name].append(round(timed(f, reps=reps), 2))
        us = {name: min(v) for name, v in runs.items()}
        x64 = xd.double().requires_grad_()
        (exact, ) = torch.autograd.grad(torch.nn.functional.layer_norm(x64, (width, ), gamma.double(), beta.double(), EPS), x64, gy.double())
        x64 = x64.detach()
        xhat = (x64 - x64.mean(dim=1, keepdim=True)) / torch.sqrt(x64.var(dim=1, unbiased=False, keepdim=True) + EPS)
        exact_gamma = (gy.double() * xhat).sum(dim=0)
        error = {}
        for name, layer in layers.items():
            gx, gw, _ = step(layer)
            error[name] = {'input_gradient': round(float((gx.double() - exact).norm() / exact.norm()), 5),
                           'gamma_gradient': round(float((gw.double() - exact_gamma).norm() / exact_gamma.norm()), 5)}
        kernels = {}
        for bits in BITS:
            kept = cabi_x.norm_state_bytes(ROWS, width, bits)
            moved = 2 * size * n + kept + 4 * ROWS                   # forward: x + y + state + rstd; backward: gy + state + rstd + dx
            floor = moved / PEAK_BYTES_PER_US
            kernels[str(bits)] = {'bytes_moved': moved, 'byte_floor_us_at_8TBs': round(floor, 2), 'forward_us': us[f'forward_{bits}'], 'backward_us': us[f'backward_{bits}'],
                                  'forward_fraction_of_floor': round(floor / us[f'forward_{bits}'], 3),
                                  'backward_fraction_of_floor': round(floor / us[f'backward_{bits}'], 3)}
        row = {'rows': ROWS, 'width': width, 'dtype': str(dtype).replace('torch.', ''),
               'us_forward_plus_backward': {name: us[name] for name in layers}, 'runs_us': runs,
               'over_nn_layer_norm': {name: round(us[name] / us['nn_layer_norm'], 4) for name in layers},
               'saved_for_backward_bytes': {name: saved_bytes(lambda layer=layer: layer(x)) for name, layer in layers.items()},
               'input_bytes': size * n, 'kept_of_the_input_bytes': {str(bits): cabi_x.norm_state_bytes(ROWS, width, bits) + 4 * ROWS for bits in BITS},
               'plain_forward_us': us['forward_plain'], 'relative_error_of_one_call': error, 'kernels': kernels}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del arms, layers, x, gy, xd, y, dx, state, workspace, exact, x64, xhat
        torch.cuda.empty_cache()
    record = {'what': 'python tools/layer_norm_bench.py: QuantizedLayerNorm forward + backward beside nn.LayerNorm, and the forward and backward entry '
                      'points alone; every arm in one process, alternating; us per call',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
