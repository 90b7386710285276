"""The sampled DCT and DFT kernel pairs at 7 x 2^k, 9 x 2^k and 15 x 2^k rows on MI355X, 768 features, bf16, p = rows / 5 (rows of a
seed): per row count, in one process, the 'dct' call, the 'dft' call, the torch.fft formulation the layer would otherwise take (cast to
fp32, full transform, gather; drawn rows) and the same kernel pair at the next larger power of two (8 x 2^k or 16 x 2^k rows, p = a
fifth of those), which moves more bytes.  Median over rounds of the average of many back-to-back calls between HIP events, after the
GPU has been kept busy with the same call (tools/sketch_bench.py::timed); the arms of a row count alternate, twice, and the smaller of
the two medians is quoted.

    python tools/transform_rows_bench.py [--out FILE]        ->  profiles/transform_rows_odd.txt, or FILE
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # tools/ -> repository root
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch
from fewbit_amd import cabi, cabi_x, linear
from sketch_bench import timed

DEV = 'cuda'
FEATURES, DTYPE = 768, torch.bfloat16
FAMILIES = ((7, range(9, 14)), (9, range(8, 13)), (15, range(8, 12)))
SPLITS = {3584: '32 x 112', 7168: '64 x 112', 14336: '128 x 112', 28672: '128 x 224', 57344: '256 x 224',
          2304: '16 x 144', 4608: '32 x 144', 9216: '64 x 144', 18432: '128 x 144', 36864: '128 x 288',
          3840: '16 x 240', 7680: '32 x 240', 15360: '64 x 240', 30720: '128 x 240'}


def kernel_call(kind, m, p):
    """the call the layer makes (rows of a seed), output and workspace allocated once"""
    rows, features = m.shape
    if kind == 'dct':
        ws = torch.empty(cabi.sampled_dct_workspace_bytes(rows, features, p, m.dtype), dtype=torch.uint8, device=DEV)
        out = torch.empty(p, features, dtype=m.dtype, device=DEV)
        return lambda: cabi.sampled_dct_seeded(m, p, 1234, rows / p, out=out, workspace=ws)
    ws = torch.empty(cabi_x.sampled_dft_workspace_bytes(rows, features, p, m.dtype), dtype=torch.uint8, device=DEV)
    out = torch.empty(2, p, features, dtype=m.dtype, device=DEV)
    return lambda: cabi_x.sampled_dft_seeded(m, p, 1234, rows / p, out=out, workspace=ws)


def torch_call(kind, m, p):
    gen = torch.Generator(device=DEV).manual_seed(3)

    def f():
        prev = linear.use_native_sketch(False)
        try:
            return linear.sampled_transform(kind, m, p, gen, scale=m.shape[0] / p)
        finally:
            linear.use_native_sketch(prev)
    return f


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'transform_rows_odd.txt'), help='where the table is written')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    lines = [f'{torch.cuda.get_device_name(0)}; {FEATURES} features, bf16, p = rows / 5, rows of a seed; us per call (median of 3 rounds of 100 calls, 20 for torch.fft; min of 2 passes)',
             f'{"rows":>7s} {"":>9s} {"split":>9s} | {"dct":>7s} {"dft":>7s} | {"torch.fft dct":>13s} {"dft":>7s} | {"x dct":>6s} {"x dft":>6s} | '
             f'{"next 2^k":>8s} {"dct":>7s} {"dft":>7s} | {"dct / next":>10s} {"dft / next":>10s}']
    for odd, ks in FAMILIES:
        for k in ks:
            rows = odd << k
            bigger = 1 << rows.bit_length()                       # 8 x 2^k, or 16 x 2^k
            assert 'fewbit_hip' in linear.sampled_transform_path('dct', torch.empty(rows, 2, device=DEV)), rows
            m = torch.randn(rows, FEATURES, device=DEV).to(DTYPE)
            mb = torch.randn(bigger, FEATURES, device=DEV).to(DTYPE)
            arms = {'dct': (kernel_call('dct', m, rows // 5), 100), 'dft': (kernel_call('dft', m, rows // 5), 100),
                    'torch dct': (torch_call('dct', m, rows // 5), 20), 'torch dft': (torch_call('dft', m, rows // 5), 20),
                    'next dct': (kernel_call('dct', mb, bigger // 5), 100), 'next dft': (kernel_call('dft', mb, bigger // 5), 100)}
            us = {}
            for _ in range(2):                                   # alternating: every arm sees the same state of the machine
                for name, (f, reps) in arms.items():
                    us[name] = min(us.get(name, float('inf')), timed(f, reps=reps))
            lines.append(f'{rows:7d} {f"= {odd} x 2^{k}":>9s} {SPLITS[rows]:>9s} | {us["dct"]:7.1f} {us["dft"]:7.1f} | {us["torch dct"]:13.1f} {us["torch dft"]:7.1f} | '
                         f'{us["torch dct"] / us["dct"]:6.1f} {us["torch dft"] / us["dft"]:6.1f} | {bigger:8d} {us["next dct"]:7.1f} {us["next dft"]:7.1f} | '
                         f'{us["dct"] / us["next dct"]:10.3f} {us["dft"] / us["next dft"]:10.3f}')
            print(lines[-1], flush=True)
            del m, mb, arms
            torch.cuda.empty_cache()
    lines.append('x dct, x dft: torch.fft formulation / kernel pair.  dct / next, dft / next: the call at m x 2^k rows over the call at the next power of two.')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines[:2]))


if __name__ == '__main__':
    main()
