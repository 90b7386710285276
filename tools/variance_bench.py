"""The variance estimator's postprocess (fewbit_amd/variance.py) on MI355X at the shapes of RoBERTa-base's linear layers: 16384 rows,
768 x 3072 and 3072 x 768 features, bf16 and fp32.  Arms per case, alternating in one process:
  (a) postprocess on the gfx950 kernels: cabi_x.row_moments + one GEMM in the operands' dtype + cabi_x.sum_squares;
  (b) the formulation it replaced: fp32 copies of both operands and the three estimate_* functions (three fp32 GEMMs, four norms);
  (c) postprocess with use_native_sketch(False): the float64 PyTorch arithmetic every other input takes;
and the one-pass kernel alone against what reads the same bytes:
  (d) cabi_x.row_moments;
  (e) two torch.linalg.vector_norm(., dim=1) calls, one per operand.
Timing as tools/sketch_bench.py::timed: the GPU is kept busy with the same call until it has settled, then the median over rounds of
many back-to-back calls between HIP events; the arms alternate twice and the smaller median is quoted.  Byte floor of (d):
rows * (n * size_x + m * size_g) at 8 TB/s.

    python tools/variance_bench.py [--out FILE]        ->  profiles/variance_bench.json
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
from fewbit_amd import cabi_x, variance
from sketch_bench import timed

DEV = 'cuda'
ROWS = 16384
CASES = tuple((n, m, dtype) for n, m in ((768, 3072), (3072, 768)) for dtype in (torch.bfloat16, torch.float32))
PEAK_BYTES_PER_US = 8.0e6


def state_of(x, g):
    state = variance._VarianceState()
    state.input, state.grad_output, state.bs, state.bs_proj = x, g, ROWS, ROWS // 5
    return state


def replaced(x, g):
    xf, gf = x.float(), g.float()
    return variance.estimate_correlation(xf, gf), variance.estimate_variance_sgd(xf, gf, ROWS), variance.estimate_variance_rmm(xf, gf, ROWS // 5)


def switched_off(state):
    prev = fewbit.linear.use_native_sketch(False)
    try:
        state.postprocess()
    finally:
        fewbit.linear.use_native_sketch(prev)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'variance_bench.json'), help='where the record is written')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    rows = []
    for n, m, dtype in CASES:
        x = torch.randn(ROWS, n, device=DEV).to(dtype)
        g = torch.randn(ROWS, m, device=DEV).to(dtype)
        state = state_of(x, g)
        out3 = torch.empty(3, dtype=torch.float64, device=DEV)
        ws = torch.empty(cabi_x.moments_workspace_bytes(ROWS, n, m), dtype=torch.uint8, device=DEV)
        arms = {
            'native_postprocess': (state.postprocess, 50),
            'replaced_formulation': (lambda: replaced(x, g), 10),
            'float64_postprocess': (lambda: switched_off(state), 3),
            'row_moments': (lambda: cabi_x.row_moments(x, g, out=out3, workspace=ws), 100),
            'two_vector_norms': (lambda: (torch.linalg.vector_norm(x, dim=1), torch.linalg.vector_norm(g, dim=1)), 100),
        }
        runs = {name: [] for name in arms}
        for _ in range(2):
            for name, (f, reps) in arms.items():
                runs[name].append(round(timed(f, reps=reps), 2))
        us = {name: min(v) for name, v in runs.items()}
        floor_bytes = ROWS * (n + m) * x.element_size()
        floor_us = floor_bytes / PEAK_BYTES_PER_US
        row = {'rows': ROWS, 'n': n, 'm': m, 'dtype': str(dtype).replace('torch.', ''), 'path': variance.variance_path(x, g), 'us': us, 'runs_us': runs,
               'native_over_replaced': round(us['native_postprocess'] / us['replaced_formulation'], 4),
               'row_moments_over_two_vector_norms': round(us['row_moments'] / us['two_vector_norms'], 4),
               'row_moments_byte_floor_bytes': floor_bytes, 'row_moments_byte_floor_us_at_8TBs': round(floor_us, 2),
               'row_moments_fraction_of_floor': round(floor_us / us['row_moments'], 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del state, arms, x, g
        torch.cuda.empty_cache()
    record = {'what': 'python tools/variance_bench.py: _VarianceState.postprocess and cabi_x.row_moments, every arm in one process, alternating; us per call',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'rows': rows,
              'verdict': {'native_postprocess_faster_than_replaced_at_every_shape': all(r['native_over_replaced'] < 1.0 for r in rows),
                          'row_moments_no_slower_than_two_vector_norms_at_every_shape': all(r['row_moments_over_two_vector_norms'] <= 1.0 for r in rows)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    print(json.dumps(record['verdict']))


if __name__ == '__main__':
    main()
