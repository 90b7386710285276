"""layer_norm_linear_mx with a residual (fewbit_amd/norm.py, the fused pair of fewbit_amd/csrc/fewbit_mxlnorm.hip) on MI355X at 16384 tokens,
768 -> (3072, ) (RoBERTa's attention output norm and the intermediate dense) and 4096 -> (4096, 1024, 1024), bf16 and fp16, fp4, p = 0 and 0.1,
post-norm (return_normed: y goes on, a gradient arrives at it) and pre-norm (prenorm: h goes on).  Arms per case, alternating in one process:
  the node forward + backward (torch.autograd.grad of the input, the residual, the norm's parameters and the weights on random gradients) beside what
  it replaces, fewbit.functional.dropout_add followed by layer_norm_linear_mx without a residual, and beside torch (F.dropout, +, F.layer_norm,
  F.linear);
  each new kernel alone, into preallocated outputs, beside the kernels it replaces on the same tensors:
    cabi_x.mx_add_layer_norm_forward beside cabi_x.dropout_apply with the residual as addend (p = 0: torch.add) + cabi_x.mx_layer_norm_forward,
    cabi_x.mx_add_layer_norm_backward beside gy.add_(at_y) (post-norm) + cabi_x.mx_layer_norm_backward + the add of gh (pre-norm) +
    cabi_x.dropout_apply of the sum (p > 0).
Timing as tools/sketch_bench.py::timed (HIP events around many back-to-back calls after the GPU has settled, median over rounds); the arms alternate
twice and the smaller median is quoted.  Beside the times: the allocator's peak over one backward of the three layers and the bytes each keeps a token.

    python tools/mx_add_layer_norm_bench.py [--out FILE]        ->  profiles/mx_add_layer_norm_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # tools/ -> repository root
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch
import torch.nn.functional as F
import fewbit_amd as fewbit
from fewbit_amd import cabi_x
from mx_add_norm_bench import backward_peak
from sketch_bench import timed

DEV = 'cuda'
TOKENS, SEED, EPS, FMT = 16384, 2026, 1e-5, 'fp4'
CASES = tuple((width, outs, dtype) for width, outs in ((4096, (4096, 1024, 1024)), (768, (3072, ))) for dtype in (torch.bfloat16, torch.float16))
SETTINGS = {f'p{str(p).replace(".", "")}_{form}': (p, form == 'prenorm') for p in (0.0, 0.1) for form in ('postnorm', 'prenorm')}


def kept_bytes(forward, parameters):
    """bytes that one forward keeps for backward, each buffer once; the parameters are not counted: they exist anyway"""
    seen, theirs = {}, {t.data_ptr() for t in parameters}
    with torch.autograd.graph.saved_tensors_hooks(lambda t: seen.setdefault(t.data_ptr(), t), lambda t: t):
        forward()
    return sum(t.numel() * t.element_size() for at, t in seen.items() if at not in theirs)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mx_add_layer_norm_bench.json'), help='where the record is written')
    ap.add_argument('--reps', type=int, default=10, help='back-to-back calls per timed round')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    rows = []
    for width, outs, dtype in CASES:
        torch.manual_seed(0)
        gamma = (1 + 0.1 * torch.randn(width, device=DEV)).to(dtype).requires_grad_()
        beta = (0.1 * torch.randn(width, device=DEV)).to(dtype).requires_grad_()
        weights = [(torch.randn(n, width, device=DEV) * width**-0.5).to(dtype).requires_grad_() for n in outs]
        x, r = (torch.randn(TOKENS, width, device=DEV).to(dtype).requires_grad_() for _ in range(2))
        g_outs, g_row = [torch.randn(TOKENS, n, device=DEV).to(dtype) for n in outs], torch.randn(TOKENS, width, device=DEV).to(dtype)
        leaves = (x, r, gamma, beta, *weights)
        xd, rd, gd, bd = x.detach(), r.detach(), gamma.detach(), beta.detach()
        gy = torch.randn(TOKENS, width, device=DEV).to(dtype)
        y, h, out, out2, g = (torch.empty_like(xd) for _ in range(5))
        rstd, mean, dgamma, dbeta = (torch.empty(n, device=DEV) for n in (TOKENS, TOKENS, width, width))
        space = torch.empty(cabi_x.mx_layer_norm_workspace(TOKENS, width), dtype=torch.uint8, device=DEV)
        cells = cabi_x.mx_layer_norm_forward(xd, gd, bd, EPS, FMT, SEED)[1]
        for setting, (p, prenorm) in SETTINGS.items():
            normed = not prenorm
            grads = [g_row, *g_outs] if normed else [*g_outs, g_row]
            fused = lambda: fewbit.functional.layer_norm_linear_mx(x, gamma, beta, weights, None, EPS, FMT, None, normed, r, p, True, prenorm)

            def composed():
                s = fewbit.functional.dropout_add(x, r, p)
                res = fewbit.functional.layer_norm_linear_mx(s, gamma, beta, weights, None, EPS, FMT, None, normed)
                return (*res, s) if prenorm else res

            def plain():
                s = r + F.dropout(x, p)
                n = F.layer_norm(s, (width, ), gamma, beta, EPS)
                res = tuple(F.linear(n, w) for w in weights)
                return (*res, s) if prenorm else (n, *res)

            step = lambda forward: torch.autograd.grad(forward(), leaves, grads)
            at_y, arriving = (g_row, None) if normed else (None, g_row)

            def old_forward():
                torch.add(rd, xd, out=h) if p == 0 else cabi_x.dropout_apply(xd, SEED + 1, p, addend=rd, out=h)
                cabi_x.mx_layer_norm_forward(h, gd, bd, EPS, FMT, SEED, y=y, mean=mean, rstd=rstd, cells=cells)

            def old_backward():
                upstream = torch.add(gy, at_y, out=g) if normed else gy
                cabi_x.mx_layer_norm_backward(upstream, cells, rstd, gd, FMT, dx=out, dgamma=dgamma, dbeta=dbeta, workspace=space)
                if prenorm:
                    out.add_(g_row)
                if p > 0:
                    cabi_x.dropout_apply(out, SEED + 1, p, out=out2)

            arms = {'layer_fused': (lambda: step(fused), args.reps), 'layer_composed': (lambda: step(composed), args.reps),
                    'layer_torch': (lambda: step(plain), args.reps),
                    'forward_fused': (lambda: cabi_x.mx_add_layer_norm_forward(xd, rd, gd, bd, EPS, FMT, (SEED, SEED + 1), p, prenorm, y, h, rstd, cells, mean),
                                      2 * args.reps),
                    'forward_replaced': (old_forward, 2 * args.reps),
                    'backward_fused': (lambda: cabi_x.mx_add_layer_norm_backward(gy, cells, rstd, gd, FMT, SEED + 1, p, arriving, (True, True, True, True), at_y, out,
                                                                                 out2 if p > 0 else None, dgamma, dbeta, space), 2 * args.reps),
                    'backward_replaced': (old_backward, 2 * args.reps)}
            runs = {name: [] for name in arms}
            for f, _ in arms.values():                           # every arm once before any is timed: allocator, code objects, clocks
                timed(f, reps=3, rounds=1)
            for _ in range(2):
                for name, (f, reps) in arms.items():
                    runs[name].append(round(timed(f, reps=reps), 2))
            us = {name: min(v) for name, v in runs.items()}
            row = {'tokens': TOKENS, 'width': width, 'outs': list(outs), 'dtype': str(dtype).replace('torch.', ''), 'format': FMT, 'setting': setting, 'us': us,
                   'runs_us': runs, 'fused_over_replaced': {k: round(us[f'{k}_fused'] / us[f'{k}_composed' if k == 'layer' else f'{k}_replaced'], 4)
                                                            for k in ('layer', 'forward', 'backward')},
                   'fused_over_torch': round(us['layer_fused'] / us['layer_torch'], 4),
                   'backward_peak_bytes': {name: backward_peak(f, leaves, grads) for name, f in (('fused', fused), ('composed', composed), ('torch', plain))},
                   'kept_bytes_per_token': {name: round(kept_bytes(f, leaves[2:]) / TOKENS, 1) for name, f in (('fused', fused), ('composed', composed), ('torch', plain))}}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del gamma, beta, weights, x, r, leaves, xd, rd, gd, bd, gy, y, h, out, out2, g, cells, space, arms, g_outs, g_row, grads
        torch.cuda.empty_cache()
    record = {'what': 'python tools/mx_add_layer_norm_bench.py: layer_norm_linear_mx with a residual (p = 0 and 0.1, post-norm with return_normed and pre-norm; '
                      'fp4) forward + backward beside dropout_add + layer_norm_linear_mx and beside torch, and cabi_x.mx_add_layer_norm_forward / '
                      '_backward alone beside the kernels they replace; every arm in one process, alternating; us per call; the allocator\'s peak over '
                      'one backward; bytes kept per token beside the parameters',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
