"""The sampled DCT and DFT with the signs of the seed (cabi_x.sampled_*_signed) beside the unsigned calls they extend
(cabi_x.sampled_*_zext_seeded, valid_rows = rows) on MI355X: 16384 x 768 and 16384 x 3072, p = 3276, bf16 and fp32.

    python tools/signed_transform_bench.py [--out FILE]                 HIP events around back-to-back calls (tools/sketch_bench.py::timed: settled,
                                                                        median of 3 rounds of 100 calls), the two arms alternating twice, the
                                                                        smaller median quoted  ->  profiles/signed_transform_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o signed -- python tools/signed_transform_bench.py --trace
                                                                        the same calls for the profiler: per case 1 s of settling, then 100 calls per arm
    python tools/signed_transform_bench.py --merge DIR [--out FILE]     adds the per-pass kernel times of that trace (the last 100 dispatches of each
                                                                        kernel and grid) to FILE
Pass B is one kernel for both arms (the signs end in pass A); pass A differs in its name (SignedRowsOfSeed / RowsOfSeed).
"""
import argparse
import collections
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

ROWS, PROJ, REPS = 16384, 3276, 100
CASES = tuple((features, dtype) for features in (768, 3072) for dtype in ('bf16', 'fp32'))


def calls(kind, m, p):
    """-> (the unsigned call, the signed call) on preallocated buffers"""
    import torch
    from fewbit_amd import cabi_x
    rows, features = m.shape
    ws = torch.empty(cabi_x.sampled_dft_workspace_bytes(rows, features, p, m.dtype), dtype=torch.uint8, device=m.device)
    out = torch.empty((p, features) if kind == 'dct' else (2, p, features), dtype=m.dtype, device=m.device)
    if kind == 'dct':
        return (lambda: cabi_x.sampled_dct_zext_seeded(m, rows, p, 1234, rows / p, out=out, workspace=ws),
                lambda: cabi_x.sampled_dct_signed(m, rows, p, 1234, rows / p, out=out, workspace=ws))
    return (lambda: cabi_x.sampled_dft_zext_seeded(m, rows, p, 1234, rows / p, out=out, workspace=ws),
            lambda: cabi_x.sampled_dft_signed(m, rows, p, 1234, rows / p, out=out, workspace=ws))


def measure(trace: bool):
    import torch
    from sketch_bench import timed
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    cases = []
    for features, dtype in CASES:
        m = torch.randn(ROWS, features, device='cuda').to({'bf16': torch.bfloat16, 'fp32': torch.float32}[dtype])
        for kind in ('dct', 'dft'):
            unsigned, signed = calls(kind, m, PROJ)
            if trace:
                t0 = time.perf_counter()
                while time.perf_counter() - t0 < 1.0:
                    unsigned(), signed()
                    torch.cuda.synchronize()
                for f in (unsigned, signed):
                    for _ in range(REPS):
                        f()
                    torch.cuda.synchronize()
                continue
            us = {}
            for _ in range(2):
                for name, f in (('unsigned', unsigned), ('signed', signed)):
                    us[name] = min(us.get(name, float('inf')), timed(f, reps=REPS))
            cases.append({'kind': kind, 'rows': ROWS, 'features': features, 'p': PROJ, 'dtype': dtype, 'unsigned_us': round(us['unsigned'], 2),
                          'signed_us': round(us['signed'], 2), 'signed_over_unsigned': round(us['signed'] / us['unsigned'], 4)})
            print(json.dumps(cases[-1]), flush=True)
        del m
    return {'device': torch.cuda.get_device_name(0), 'what': 'cabi_x.sampled_*_signed against cabi_x.sampled_*_zext_seeded (valid_rows = rows); HIP events, us per call, '
            'median of 3 rounds of 100 calls after settling, the arms alternating twice, the smaller median', 'cases': cases}


def merge(trace_dir: str, result: dict) -> dict:
    """per-pass kernel times of a rocprofv3 --kernel-trace run of --trace: the mean and the least of the last REPS dispatches of each (kernel, grid)"""
    hits = sorted(glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True))
    assert hits, f'no kernel trace under {trace_dir}'
    per = collections.defaultdict(list)
    with open(hits[0], newline='') as f:
        for row in csv.DictReader(f):
            name = row['Kernel_Name']
            if 'pass_a_zext_kernel' in name or 'pass_b_kernel' in name:
                per[name, int(row['Grid_Size_Y']) // max(int(row.get('Workgroup_Size_Y', 1) or 1), 1)].append(int(row['End_Timestamp']) - int(row['Start_Timestamp']))
    # (every kernel and grid of the trace, so that a reader can check the assignment below)
    result['trace'] = [{'kernel': name[:name.index('(')] if '(' in name else name, 'grid_y': y, 'dispatches': len(spans), 'mean_us_last_100': round(sum(spans[-REPS:]) / len(spans[-REPS:]) / 1e3, 2)}
                       for (name, y), spans in sorted(per.items())]
    dt = {'fp32': 0, 'bf16': 2}
    for case in result['cases']:
        tiles, halves = (case['features'] + 63) // 64, (case['features'] + 31) // 32
        order, epilogue = ('RowsMakhoul', 'CosineRows') if case['kind'] == 'dct' else ('RowsInOrder', 'FourierPlanes')
        kernels = {}
        for (name, y), spans in per.items():
            args = name[name.index('<') + 1:]
            if 'pass_a_zext_kernel' in name and order in name and y == tiles and args.split(',')[1].strip() == str(dt[case['dtype']]):
                key = 'pass_a_signed_us' if 'SignedRowsOfSeed' in name else 'pass_a_unsigned_us'
            elif 'pass_b_kernel' in name and epilogue in name and y == halves and args.split(',')[1].strip() == str(dt[case['dtype']]):
                key = 'pass_b_us'                      # (one kernel for both arms: 2 x REPS dispatches)
            else:
                continue
            last = spans[-(2 * REPS if key == 'pass_b_us' else REPS):]
            kernels[key] = round(sum(last) / len(last) / 1e3, 2)
            kernels[key.replace('_us', '_min_us')] = round(min(last) / 1e3, 2)
            kernels[key.replace('_us', '_dispatches')] = len(last)
        if 'pass_a_signed_us' in kernels and 'pass_a_unsigned_us' in kernels:
            kernels['pass_a_signed_over_unsigned'] = round(kernels['pass_a_signed_us'] / kernels['pass_a_unsigned_us'], 4)
        case['kernels'] = kernels
    result['kernels'] = 'rocprofv3 --kernel-trace --stats over --trace: us per dispatch, mean and least of the last 100 dispatches of each kernel (pass B: 200, one kernel for both arms)'
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'signed_transform_bench.json'))
    ap.add_argument('--trace', action='store_true', help='only run the calls (under rocprofv3)')
    ap.add_argument('--merge', default=None, metavar='DIR', help='add the kernel times of the rocprofv3 trace under DIR to --out')
    args = ap.parse_args()
    if args.trace:
        measure(True)
        return
    if args.merge:
        with open(args.out) as f:
            result = merge(args.merge, json.load(f))
    else:
        result = measure(False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(result, indent=1) + '\n')


if __name__ == '__main__':
    main()
