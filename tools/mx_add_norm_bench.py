"""rms_norm_linear_mx with a residual (fewbit_amd/norm.py, the fused pair of fewbit_amd/csrc/fewbit_mxnorm.hip) on MI355X at 16384 tokens,
4096 -> (4096, 1024, 1024) and 768 -> (768, 768, 768), bf16 and fp16, fp4 and fp6, in the two settings a block runs: p = 0 with prenorm (the Llama
family) and p = 0.1 post-norm (T5).  Arms per case, alternating in one process:
  the node forward + backward (torch.autograd.grad of the input, the residual, the norm's weight and the three weights on random gradients, one of them
  arriving at h with prenorm) beside what it replaces, fewbit.functional.dropout_add followed by rms_norm_linear_mx without a residual;
  each new kernel alone, into preallocated outputs, beside the kernels it replaces on the same tensors:
    cabi_x.mx_add_rms_norm_forward beside cabi_x.dropout_apply with the residual as addend (p = 0: torch.add) + cabi_x.mx_rms_norm_forward,
    cabi_x.mx_add_rms_norm_backward beside cabi_x.mx_rms_norm_backward + the add of gh (prenorm) + cabi_x.dropout_apply of the sum (p > 0).
Timing as tools/sketch_bench.py::timed (HIP events around many back-to-back calls after the GPU has settled, median over rounds); the arms alternate
twice and the smaller median is quoted.  Beside the times: the allocator's peak over one backward of both layers.

    python tools/mx_add_norm_bench.py [--out FILE]        ->  profiles/mx_add_norm_bench.json
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
SETTINGS = {'p0_prenorm': (0.0, True), 'p01_postnorm': (0.1, False)}


def backward_peak(forward, leaves, grads):
    """bytes by which the allocator's peak over ONE backward exceeds what was allocated before it"""
    outs = forward()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    torch.autograd.grad(outs, leaves, grads[:len(outs)])
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mx_add_norm_bench.json'), help='where the record is written')
    ap.add_argument('--reps', type=int, default=10, help='back-to-back calls per timed round')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    rows = []
    for width, outs, dtype in CASES:
        torch.manual_seed(0)
        gamma = (1 + 0.1 * torch.randn(width, device=DEV)).to(dtype).requires_grad_()
        weights = [(torch.randn(n, width, device=DEV) * width**-0.5).to(dtype).requires_grad_() for n in outs]
        x, r = (torch.randn(TOKENS, width, device=DEV).to(dtype).requires_grad_() for _ in range(2))
        grads = [torch.randn(TOKENS, n, device=DEV).to(dtype) for n in (*outs, width)]
        leaves = (x, r, gamma, *weights)
        xd, rd, gd, gy, gh = x.detach(), r.detach(), gamma.detach(), grads[0], grads[3]
        y, h, out, out2 = (torch.empty_like(xd) for _ in range(4))
        rstd, dgamma = torch.empty(TOKENS, device=DEV), torch.empty(width, device=DEV)
        space = torch.empty(cabi_x.mx_rms_norm_workspace(TOKENS, width), dtype=torch.uint8, device=DEV)
        for fmt in FORMATS:
            cells = cabi_x.mx_rms_norm_forward(xd, gd, EPS, fmt, SEED)[1]
            for setting, (p, prenorm) in SETTINGS.items():
                fused = lambda: fewbit.functional.rms_norm_linear_mx(x, gamma, weights, None, EPS, fmt, residual=r, p=p, prenorm=prenorm)

                def composed():
                    s = fewbit.functional.dropout_add(x, r, p)
                    res = fewbit.functional.rms_norm_linear_mx(s, gamma, weights, None, EPS, fmt)
                    return (*res, s) if prenorm else res

                step = lambda forward: torch.autograd.grad(forward(), leaves, grads[:4 if prenorm else 3])
                arriving = gh if prenorm else None

                def old_forward():
                    torch.add(rd, xd, out=h) if p == 0 else cabi_x.dropout_apply(xd, SEED + 1, p, addend=rd, out=h)
                    cabi_x.mx_rms_norm_forward(h, gd, EPS, fmt, SEED, y=y, rstd=rstd, cells=cells)

                def old_backward():
                    cabi_x.mx_rms_norm_backward(gy, cells, rstd, gd, fmt, dx=out, dgamma=dgamma, workspace=space)
                    if prenorm:
                        out.add_(gh)
                    if p > 0:
                        cabi_x.dropout_apply(out, SEED + 1, p, out=out2)

                arms = {'layer_fused': (lambda: step(fused), args.reps), 'layer_composed': (lambda: step(composed), args.reps),
                        'forward_fused': (lambda: cabi_x.mx_add_rms_norm_forward(xd, rd, gd, EPS, fmt, (SEED, SEED + 1), p, prenorm, y, h, rstd, cells), 2 * args.reps),
                        'forward_replaced': (old_forward, 2 * args.reps),
                        'backward_fused': (lambda: cabi_x.mx_add_rms_norm_backward(gy, cells, rstd, gd, fmt, SEED + 1, p, arriving, (True, True, True), out,
                                                                                   out2 if p > 0 else None, dgamma, space), 2 * args.reps),
                        'backward_replaced': (old_backward, 2 * args.reps)}
                runs = {name: [] for name in arms}
                for f, _ in arms.values():                           # every arm once before any is timed: allocator, code objects, clocks
                    timed(f, reps=3, rounds=1)
                for _ in range(2):
                    for name, (f, reps) in arms.items():
                        runs[name].append(round(timed(f, reps=reps), 2))
                us = {name: min(v) for name, v in runs.items()}
                row = {'tokens': TOKENS, 'width': width, 'outs': list(outs), 'dtype': str(dtype).replace('torch.', ''), 'format': fmt, 'setting': setting, 'us': us,
                       'runs_us': runs, 'fused_over_replaced': {k: round(us[f'{k}_fused'] / us[f'{k}_composed' if k == 'layer' else f'{k}_replaced'], 4)
                                                                for k in ('layer', 'forward', 'backward')},
                       'backward_peak_bytes': {'fused': backward_peak(fused, leaves, grads), 'composed': backward_peak(composed, leaves, grads)}}
                rows.append(row)
                print(json.dumps(row), flush=True)
        del gamma, weights, x, r, grads, leaves, xd, rd, gd, gy, gh, y, h, out, out2, cells, space, arms
        torch.cuda.empty_cache()
    record = {'what': 'python tools/mx_add_norm_bench.py: rms_norm_linear_mx with a residual (p = 0 with prenorm, p = 0.1 post-norm; fp4, fp6) forward + backward '
                      'beside dropout_add + rms_norm_linear_mx, and cabi_x.mx_add_rms_norm_forward / mx_add_rms_norm_backward alone beside the kernels they '
                      'replace; every arm in one process, alternating; us per call; the allocator\'s peak over one backward',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
