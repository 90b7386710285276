"""The zero-extended sampled DCT and DFT (cabi_x.sampled_*_zext_seeded) on MI355X at 12800 and 51200 rows (N' = 14336 and 57344), 768 and
3072 features, bf16 and fp32, p = rows / 5, rows of a seed.  Four arms per case, interleaved in one process:
  (a) the zero-extended call on the N rows;
  (b) F.pad to N' rows + the plain call (the copy is written, re-read and allocated);
  (c) the plain call on N' real rows (same arithmetic, more bytes loaded);
  (d) the torch.fft formulation at N (what the layer takes with the switch off).
Timing as tools/transform_rows_bench.py: median over rounds of many back-to-back calls between HIP events (tools/sketch_bench.py::timed),
the arms alternate twice and the smaller median is quoted.

    python tools/transform_zext_bench.py [--out FILE]        ->  profiles/transform_zext.txt (and its row of profiles/README.md, through
                                                                tools/profiles_index.py), or FILE
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # tools/ -> repository root
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch
import torch.nn.functional as F
from fewbit_amd import cabi, cabi_x
import profiles_index
from sketch_bench import timed
from transform_rows_bench import kernel_call, torch_call

DEV = 'cuda'
CASES = tuple((rows, features, dtype) for rows in (12800, 51200) for features in (768, 3072) for dtype in (torch.bfloat16, torch.float32))


def zext_call(kind, m, big, p):
    features = m.shape[1]
    ws = torch.empty(cabi_x.sampled_dft_workspace_bytes(big, features, p, m.dtype), dtype=torch.uint8, device=DEV)
    if kind == 'dct':
        out = torch.empty(p, features, dtype=m.dtype, device=DEV)
        return lambda: cabi_x.sampled_dct_zext_seeded(m, big, p, 1234, big / p, out=out, workspace=ws)
    out = torch.empty(2, p, features, dtype=m.dtype, device=DEV)
    return lambda: cabi_x.sampled_dft_zext_seeded(m, big, p, 1234, big / p, out=out, workspace=ws)


def padded_call(kind, m, big, p):
    features = m.shape[1]
    ws = torch.empty(cabi.sampled_dct_workspace_bytes(big, features, p, m.dtype), dtype=torch.uint8, device=DEV)
    if kind == 'dct':
        out = torch.empty(p, features, dtype=m.dtype, device=DEV)
        return lambda: cabi.sampled_dct_seeded(F.pad(m, (0, 0, 0, big - m.shape[0])), p, 1234, big / p, out=out, workspace=ws)
    out = torch.empty(2, p, features, dtype=m.dtype, device=DEV)
    return lambda: cabi_x.sampled_dft_seeded(F.pad(m, (0, 0, 0, big - m.shape[0])), p, 1234, big / p, out=out, workspace=ws)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'transform_zext.txt'), help='where the table is written')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    lines = [f'{torch.cuda.get_device_name(0)}; p = rows / 5, rows of a seed; us per call (median of 3 rounds of 100 calls, 20 for torch.fft; min of 2 passes)',
             f'{"kind":>4s} {"rows":>6s} {"at":>6s} {"feat":>5s} {"dtype":>8s} | {"(a) zext":>9s} {"(b) pad+call":>12s} {"(c) real N\'":>11s} {"(d) torch.fft":>13s} | '
             f'{"a / c":>6s} {"a / b":>6s} {"d / a":>6s}']
    for rows, features, dtype in CASES:
        big, p = cabi_x.sampled_rows_ceil(rows), rows // 5
        m = torch.randn(rows, features, device=DEV).to(dtype)
        mb = torch.randn(big, features, device=DEV).to(dtype)
        for kind in ('dct', 'dft'):
            real = kernel_call(kind, mb, p)
            arms = {'a': (zext_call(kind, m, big, p), 100), 'b': (padded_call(kind, m, big, p), 100), 'c': (real, 100), 'd': (torch_call(kind, m, p), 20)}
            us = {}
            for _ in range(2):
                for name, (f, reps) in arms.items():
                    us[name] = min(us.get(name, float('inf')), timed(f, reps=reps))
            lines.append(f'{kind:>4s} {rows:6d} {big:6d} {features:5d} {str(dtype).replace("torch.", ""):>8s} | {us["a"]:9.1f} {us["b"]:12.1f} {us["c"]:11.1f} {us["d"]:13.1f} | '
                         f'{us["a"] / us["c"]:6.3f} {us["a"] / us["b"]:6.3f} {us["d"] / us["a"]:6.1f}')
            print(lines[-1], flush=True)
            del arms
        del m, mb
        torch.cuda.empty_cache()
    lines.append("a / c: the zero-extended call over the plain call on N' real rows (it loads N / N' of the input; not slower beyond the +- 2 % between boxes is the "
                 'expectation).  a / b and d / a: reported.')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    if os.path.dirname(os.path.abspath(args.out)) == os.path.join(ROOT, 'profiles'):
        sys.argv[1:] = []                                   # (profiles_index reads its own command line: rewrite the index, not --check)
        rc = profiles_index.main()                          # fails when the file has no row
        assert rc == 0, 'tools/profiles_index.py has no row for ' + os.path.basename(args.out)


if __name__ == '__main__':
    main()
