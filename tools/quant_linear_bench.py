"""QuantizedLinear (fewbit_amd/linear.py, fewbit_amd/csrc/fewbit_quant.hip) on MI355X at the shapes of RoBERTa-base's two MLP linears, 16384 rows,
768 -> 3072 and 3072 -> 768, bf16 and fp32.  Arms per case, alternating in one process, each forward + backward (torch.autograd.grad of the
input, the weight and the bias on a random gradient):
  (a) torch.nn.Linear                                              keeps its input;
  (b) fewbit.RandomizedLinear(matmul='dct', proj_dim_ratio=0.2)     keeps a projection of 0.2 x the rows;
  (c) fewbit.QuantizedLinear(bits=2 / 4 / 8)                        keeps every element in a few bits;
and the two kernels alone, into preallocated outputs, for their share of the byte floor at 8 TB/s:
  (d) cabi_x.quant_pack(x, seed, bits, out=packed)                  floor: s n + quant_bytes(n, bits) bytes (read x, write the buffer);
  (e) cabi_x.quant_unpack(packed, n, bits, dtype, out=out)          floor: quant_bytes(n, bits) + s n bytes.
Timing as tools/sketch_bench.py::timed: the GPU is kept busy with the same call until it has settled, then the median over rounds of many
back-to-back calls between HIP events; the arms alternate twice and the smaller median is quoted.  Bytes saved for backward are counted with
fewbit.memory_usage_hooks (the weight included, which every arm keeps).  Beside each quantized arm: the relative error of one weight
gradient against the fp64 product, and of the 'dct' arm's.

    python tools/quant_linear_bench.py [--out FILE]        ->  profiles/quant_linear_bench.json
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
ROWS, SEED = 16384, 2026
CASES = tuple((fin, fout, dtype) for fin, fout in ((768, 3072), (3072, 768)) for dtype in (torch.bfloat16, torch.float32))
BITS = (2, 4, 8)
PEAK_BYTES_PER_US = 8.0e6


def saved_bytes(f):
    with fewbit.memory_usage_hooks() as usage:
        f()
    return usage.forward or 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'quant_linear_bench.json'), help='where the record is written')
    ap.add_argument('--reps', type=int, default=50, help='back-to-back calls per timed round')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    rows = []
    for fin, fout, dtype in CASES:
        torch.manual_seed(0)
        x = torch.randn(ROWS, fin, device=DEV).to(dtype).requires_grad_()
        gy = torch.randn(ROWS, fout, device=DEV).to(dtype)
        layers = {'nn_linear': torch.nn.Linear(fin, fout, device=DEV, dtype=dtype),
                  'dct_0.2': fewbit.RandomizedLinear(fin, fout, device=DEV, dtype=dtype, matmul='dct', proj_dim_ratio=0.2)}
        for bits in BITS:
            layers[f'quantized_{bits}'] = fewbit.QuantizedLinear(fin, fout, device=DEV, dtype=dtype, bits=bits)
        for layer in layers.values():                                 # one set of parameters
            layer.load_state_dict(layers['nn_linear'].state_dict())
        step = lambda layer: torch.autograd.grad(layer(x), (x, layer.weight, layer.bias), gy)
        arms = {name: (lambda layer=layer: step(layer), args.reps) for name, layer in layers.items()}
        n, size, xd = ROWS * fin, x.element_size(), x.detach()
        out, packed = torch.empty_like(xd), {bits: cabi_x.quant_pack(xd, SEED, bits) for bits in BITS}
        for bits in BITS:
            arms[f'pack_{bits}'] = (lambda bits=bits: cabi_x.quant_pack(xd, SEED, bits, out=packed[bits]), 2 * args.reps)
            arms[f'unpack_{bits}'] = (lambda bits=bits: cabi_x.quant_unpack(packed[bits], n, bits, dtype, out=out), 2 * args.reps)
        runs = {name: [] for name in arms}
        for f, _ in arms.values():                                   # every arm once before any is timed: allocator, code objects, clocks
            timed(f, reps=10, rounds=1)
        for _ in range(2):
            for name, (f, reps) in arms.items():
                runs[name].append(round(timed(f, reps=reps), 2))
        us = {name: min(v) for name, v in runs.items()}
        exact = gy.double().T @ xd.double()
        error = {name: round(float((step(layer)[1].double() - exact).norm() / exact.norm()), 5) for name, layer in layers.items()}
        kernels = {}
        for bits in BITS:
            moved = size * n + cabi_x.quant_bytes(n, bits)
            floor = moved / PEAK_BYTES_PER_US
            kernels[str(bits)] = {'bytes_moved': moved, 'byte_floor_us_at_8TBs': round(floor, 2), 'pack_us': us[f'pack_{bits}'], 'unpack_us': us[f'unpack_{bits}'],
                                  'pack_fraction_of_floor': round(floor / us[f'pack_{bits}'], 3), 'unpack_fraction_of_floor': round(floor / us[f'unpack_{bits}'], 3)}
        row = {'rows': ROWS, 'in_features': fin, 'out_features': fout, 'dtype': str(dtype).replace('torch.', ''),
               'us_forward_plus_backward': {name: us[name] for name in layers}, 'runs_us': runs,
               'over_nn_linear': {name: round(us[name] / us['nn_linear'], 4) for name in layers},
               'over_dct': {name: round(us[name] / us['dct_0.2'], 4) for name in layers},
               'saved_for_backward_bytes': {name: saved_bytes(lambda layer=layer: layer(x)) for name, layer in layers.items()},
               'input_bytes': size * n, 'kept_of_the_input_bytes': {str(bits): cabi_x.quant_bytes(n, bits) for bits in BITS},
               'weight_gradient_relative_error_of_one_call': error, 'kernels': kernels}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del arms, layers, x, gy, xd, out, packed, exact
        torch.cuda.empty_cache()
    record = {'what': 'python tools/quant_linear_bench.py: QuantizedLinear forward + backward beside nn.Linear and RandomizedLinear(dct, 0.2), and the '
                      'pack / unpack kernels alone; every arm in one process, alternating; us per call',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
