"""MXLinear (fewbit_amd/linear.py, fewbit_amd/csrc/fewbit_mx.hip) on MI355X at 16384 rows, 768 -> 3072, 3072 -> 768 and 4096 -> 11008, bf16 and fp16.
Arms per case, alternating in one process:
  the weight gradient alone, into preallocated outputs, on the same operands
    (a) cabi_x.mx_wgrad(G^ fp8, X^ fp4 / fp6)                       the scaled MFMA kernel, buffers packed beforehand;
    (b) the same with cabi_x.mx_pack(G, 'fp8', 'grad') in front       what the layer's backward runs;
    (c) cabi_x.mx_unpack + torch.mm on the exact G                    the route of the widths mx_wgrad does not serve;
    (d) torch.mm(G^T, X) on the full tensors;
    (e) cabi_x.quant_unpack + torch.mm at 4 bits (kept.products)      the integer form's default route;
    (f) cabi_x.quant_wgrad at 4 bits                                  the integer form's fused kernel (EXPERIMENTS 8.31);
  the pack kernel alone against its byte floor at 8 TB/s: cabi_x.mx_pack of X into fp4 / fp6 and of G into fp8 (floor: read the tensor, write mx_bytes);
  the layer forward + backward (torch.autograd.grad of the input, the weight and the bias on a random gradient):
    torch.nn.Linear, fewbit.QuantizedLinear(bits=4), fewbit.MXLinear('fp4'), fewbit.MXLinear('fp6').
Timing as tools/sketch_bench.py::timed (HIP events around many back-to-back calls after the GPU has settled, median over rounds); the arms alternate
twice and the smaller median is quoted.  Beside the times: bytes saved for backward (fewbit.memory_usage_hooks, the weight included), the allocator's
peak over one backward, and the relative error of one weight gradient against the fp64 product.

    python tools/mx_linear_bench.py [--out FILE]        ->  profiles/mx_linear_bench.json
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
from fewbit_amd import cabi_x, kept
from sketch_bench import timed

DEV = 'cuda'
ROWS, SEED = 16384, 2026
CASES = tuple((fin, fout, dtype) for fin, fout in ((768, 3072), (3072, 768), (4096, 11008)) for dtype in (torch.bfloat16, torch.float16))
FORMATS = ('fp4', 'fp6')
PEAK_BYTES_PER_US = 8.0e6


def saved_bytes(f):
    with fewbit.memory_usage_hooks() as usage:
        f()
    return usage.forward or 0


def backward_peak(layer, x, gy):
    """bytes by which the allocator's peak over ONE backward exceeds what was allocated before it"""
    y = layer(x)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    torch.autograd.grad(y, (x, layer.weight, layer.bias), gy)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mx_linear_bench.json'), help='where the record is written')
    ap.add_argument('--reps', type=int, default=30, help='back-to-back calls per timed round')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    rows = []
    for fin, fout, dtype in CASES:
        torch.manual_seed(0)
        x = torch.randn(ROWS, fin, device=DEV).to(dtype).requires_grad_()
        gy = torch.randn(ROWS, fout, device=DEV).to(dtype)
        xd, size = x.detach(), x.element_size()
        shape = (ROWS, fin, fout)
        out32 = torch.empty(fout, fin, device=DEV, dtype=torch.float32)
        out16 = torch.empty(fout, fin, device=DEV, dtype=dtype)
        decoded = torch.empty_like(xd)
        packed = {fmt: cabi_x.mx_pack(xd, SEED, fmt, 'kept') for fmt in FORMATS}
        gpacked = cabi_x.mx_pack(gy, SEED, 'fp8', 'grad')
        qpacked = cabi_x.quant_pack(xd, SEED, 4)
        spaces = {fmt: torch.empty(max(cabi_x.mx_wgrad_workspace(*shape, fmt), 16), dtype=torch.uint8, device=DEV) for fmt in FORMATS}
        qspace = torch.empty(max(cabi_x.quant_wgrad_workspace(dtype, *shape, 4), 16), dtype=torch.uint8, device=DEV)
        layers = {'nn_linear': torch.nn.Linear(fin, fout, device=DEV, dtype=dtype), 'quantized_4': fewbit.QuantizedLinear(fin, fout, device=DEV, dtype=dtype, bits=4)}
        for fmt in FORMATS:
            layers[f'mx_{fmt}'] = fewbit.MXLinear(fin, fout, device=DEV, dtype=dtype, format=fmt)
        for layer in layers.values():                                 # one set of parameters
            layer.load_state_dict(layers['nn_linear'].state_dict())
        step = lambda layer: torch.autograd.grad(layer(x), (x, layer.weight, layer.bias), gy)
        arms = {f'layer_{name}': (lambda layer=layer: step(layer), args.reps) for name, layer in layers.items()}
        arms['wgrad_torch_mm'] = (lambda: torch.mm(gy.T, xd, out=out16), args.reps)
        arms['wgrad_quant_unpack_mm_4'] = (lambda: kept.products((gy, ), (qpacked, ), (ROWS, fin), 4), args.reps)
        arms['wgrad_quant_wgrad_4'] = (lambda: cabi_x.quant_wgrad(gy, qpacked, fin, 4, torch.float32, out32, workspace=qspace), args.reps)
        arms['pack_g_fp8'] = (lambda: cabi_x.mx_pack(gy, SEED, 'fp8', 'grad', out=gpacked), 2 * args.reps)
        for fmt in FORMATS:
            arms[f'wgrad_mx_{fmt}'] = (lambda fmt=fmt: cabi_x.mx_wgrad(gpacked, packed[fmt], *shape, fmt, torch.float32, out32, workspace=spaces[fmt]), args.reps)
            arms[f'wgrad_mx_{fmt}_with_pack_of_g'] = (lambda fmt=fmt: cabi_x.mx_wgrad(cabi_x.mx_pack(gy, SEED, 'fp8', 'grad', out=gpacked), packed[fmt], *shape, fmt,
                                                                                      torch.float32, out32, workspace=spaces[fmt]), args.reps)
            arms[f'wgrad_mx_unpack_mm_{fmt}'] = (lambda fmt=fmt: torch.mm(gy.T, cabi_x.mx_unpack(packed[fmt], ROWS, fin, fmt, dtype, out=decoded), out=out16), args.reps)
            arms[f'pack_x_{fmt}'] = (lambda fmt=fmt: cabi_x.mx_pack(xd, SEED, fmt, 'kept', out=packed[fmt]), 2 * args.reps)
        runs = {name: [] for name in arms}
        for f, _ in arms.values():                                   # every arm once before any is timed: allocator, code objects, clocks
            timed(f, reps=5, rounds=1)
        for _ in range(2):
            for name, (f, reps) in arms.items():
                runs[name].append(round(timed(f, reps=reps), 2))
        us = {name: min(v) for name, v in runs.items()}
        exact = gy.double().T @ xd.double()
        error = {name: round(float((step(layer)[1].double() - exact).norm() / exact.norm()), 5) for name, layer in layers.items()}
        kernels = {}
        for name, t, fmt in [(f'pack_x_{fmt}', xd, fmt) for fmt in FORMATS] + [('pack_g_fp8', gy, 'fp8')]:
            moved = size * t.numel() + cabi_x.mx_bytes(*t.shape, fmt)
            floor = moved / PEAK_BYTES_PER_US
            kernels[name] = {'bytes_moved': moved, 'byte_floor_us_at_8TBs': round(floor, 2), 'us': us[name], 'fraction_of_floor': round(floor / us[name], 3)}
        flops = 2.0 * ROWS * fin * fout
        row = {'rows': ROWS, 'in_features': fin, 'out_features': fout, 'dtype': str(dtype).replace('torch.', ''), 'us': us, 'runs_us': runs,
               'mx_wgrad_over': {fmt: {other: round(us[f'wgrad_mx_{fmt}'] / us[other], 4) for other in ('wgrad_torch_mm', 'wgrad_quant_unpack_mm_4', 'wgrad_quant_wgrad_4',
                                                                                                         f'wgrad_mx_unpack_mm_{fmt}')} for fmt in FORMATS},
               'mx_wgrad_with_pack_of_g_over': {fmt: {other: round(us[f'wgrad_mx_{fmt}_with_pack_of_g'] / us[other], 4)
                                                      for other in ('wgrad_torch_mm', 'wgrad_quant_unpack_mm_4', 'wgrad_quant_wgrad_4', f'wgrad_mx_unpack_mm_{fmt}')} for fmt in FORMATS},
               'mx_wgrad_tflops': {fmt: round(flops / us[f'wgrad_mx_{fmt}'] / 1e6, 1) for fmt in FORMATS}, 'torch_mm_tflops': round(flops / us['wgrad_torch_mm'] / 1e6, 1),
               'plan': {'tile': list(cabi_x.MX_WGRAD_TILE), 'slices': cabi_x.mx_wgrad_slices(*shape), 'workspace_bytes': cabi_x.mx_wgrad_workspace(*shape, 'fp4')},
               'layer_over_nn_linear': {name: round(us[f'layer_{name}'] / us['layer_nn_linear'], 4) for name in layers},
               'layer_over_quantized_4': {name: round(us[f'layer_{name}'] / us['layer_quantized_4'], 4) for name in layers},
               'saved_for_backward_bytes': {name: saved_bytes(lambda layer=layer: layer(x)) for name, layer in layers.items()},
               'input_bytes': size * xd.numel(), 'kept_of_the_input_bytes': {fmt: cabi_x.mx_bytes(ROWS, fin, fmt) for fmt in FORMATS},
               'backward_peak_bytes': {name: backward_peak(layer, x, gy) for name, layer in layers.items()},
               'weight_gradient_relative_error_of_one_call': error, 'kernels': kernels}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del arms, layers, x, gy, xd, out32, out16, decoded, packed, gpacked, qpacked, spaces, qspace, exact
        torch.cuda.empty_cache()
    record = {'what': 'python tools/mx_linear_bench.py: the weight gradient alone (cabi_x.mx_wgrad with and without the pack of G, beside torch.mm, mx_unpack + mm, '
                      'quant_unpack + mm and quant_wgrad at 4 bits), cabi_x.mx_pack against its byte floor, and MXLinear forward + backward beside nn.Linear and '
                      'QuantizedLinear(bits=4); every arm in one process, alternating; us per call',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
