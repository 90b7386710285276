"""DropoutAddLayerNorm / DropoutAddRMSNorm (fewbit_amd/norm.py, fewbit_amd/csrc/fewbit_norm.hip) on MI355X: a sublayer's ending as ONE node against the
same ending composed of this project's own pieces, and against torch's.  Cases, each in bf16 and fp32:
    16384 x 768 and 16384 x 3072   layer norm, p = 0.1, post-norm      y = LN(residual + dropout(x))
    16384 x 4096                   RMS norm,  p = 0,   prenorm=True    h = residual + x, y = RMSNorm(h), a loss on both
Arms per case, alternating in one process, each forward + backward (torch.autograd.grad of input, residual and the parameters on random gradients):
  (a) fused_{2,4,8}      fewbit.DropoutAddLayerNorm / DropoutAddRMSNorm: one launch forward, two backward, one seed;
  (b) composed_{2,4,8}   fewbit.functional.dropout_add, then fewbit.QuantizedLayerNorm / QuantizedRMSNorm: two launches forward, three backward, two seeds;
  (c) torch              norm(residual + F.dropout(x, p));
and the fused entry points alone, into preallocated outputs, for their share of the byte floor at 8 TB/s:
  (d) cabi_x.add_*_norm_forward    floor: x + residual + y (+ h with prenorm) + state + rstd bytes;
  (e) cabi_x.add_*_norm_backward   floor: gy (+ gh) + state + rstd + dres (+ dbranch with a mask) bytes.
Timing as tools/sketch_bench.py::timed; the arms alternate twice and the smaller median is quoted.  Bytes saved for backward are counted with
fewbit.memory_usage_hooks.  The layer arms are bimodal between runs on one host (EXPERIMENTS.md 8.20): run the tool several times and compare minima.

    python tools/add_norm_bench.py [--out FILE]        ->  profiles/add_norm_bench.json
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
from sketch_bench import timed

DEV = 'cuda'
ROWS, SEED, EPS = 16384, 2026, 1e-5
SHAPES = ((768, True, 0.1, False), (3072, True, 0.1, False), (4096, False, 0.0, True))      # width, centred, p, prenorm
BITS = (2, 4, 8)
PEAK_BYTES_PER_US = 8.0e6


def saved_bytes(f):
    with fewbit.memory_usage_hooks() as usage:
        f()
    return usage.forward or 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'add_norm_bench.json'), help='where the record is written')
    ap.add_argument('--reps', type=int, default=50, help='back-to-back calls per timed round')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    rows = []
    for (width, centred, p, prenorm), dtype in ((shape, dtype) for shape in SHAPES for dtype in (torch.bfloat16, torch.float32)):
        torch.manual_seed(0)
        x = torch.randn(ROWS, width, device=DEV).to(dtype).requires_grad_()
        res = (3 + 2 * torch.randn(ROWS, width, device=DEV)).to(dtype).requires_grad_()
        gy, gh = torch.randn(ROWS, width, device=DEV).to(dtype), torch.randn(ROWS, width, device=DEV).to(dtype)
        base = (torch.nn.LayerNorm if centred else torch.nn.RMSNorm)(width, eps=EPS, device=DEV, dtype=dtype)
        with torch.no_grad():
            base.weight.copy_(1 + 0.5 * torch.randn(width, device=DEV))
        parameters = tuple(base.parameters())
        leaves = (x, res, *parameters)
        fused_of = fewbit.DropoutAddLayerNorm.from_layer_norm if centred else fewbit.DropoutAddRMSNorm.from_rms_norm
        plain_of = fewbit.QuantizedLayerNorm.from_layer_norm if centred else fewbit.QuantizedRMSNorm.from_rms_norm

        def finish(y, h):                                            # (pre-norm: the loss reaches y and the residual stream h)
            return torch.autograd.grad((y, h), leaves, (gy, gh)) if prenorm else torch.autograd.grad(y, leaves, gy)

        def fused_step(layer):
            out = layer(x, res)
            return finish(*out) if prenorm else finish(out, None)

        def composed_step(layer):
            h = fewbit.functional.dropout_add(x, res, p, True)
            return finish(layer(h), h)

        def torch_step():
            h = res + F.dropout(x, p, True)
            return finish(base(h), h)

        calls = {'torch': torch_step}
        for bits in BITS:
            calls[f'fused_{bits}'] = lambda layer=fused_of(base, p=p, prenorm=prenorm, bits=bits): fused_step(layer)
            calls[f'composed_{bits}'] = lambda layer=plain_of(base, bits=bits): composed_step(layer)
        arms = {name: (f, args.reps) for name, f in calls.items()}
        # the entry points alone
        n, size, xd, rd = ROWS * width, x.element_size(), x.detach(), res.detach()
        gamma = base.weight.detach()
        beta = (base.bias.detach(), ) if centred else ()
        forward = cabi_x.add_layer_norm_forward if centred else cabi_x.add_rms_norm_forward
        backward = cabi_x.add_layer_norm_backward if centred else cabi_x.add_rms_norm_backward
        mask = cabi_x.dropout_threshold(p) > 0
        y, dres, rstd = torch.empty_like(xd), torch.empty_like(xd), torch.empty(ROWS, dtype=torch.float32, device=DEV)
        h = torch.empty_like(xd) if prenorm else None
        dbranch = torch.empty_like(xd) if mask else None
        sums = {'dgamma': torch.empty(width, dtype=torch.float32, device=DEV), **({'dbeta': torch.empty(width, dtype=torch.float32, device=DEV)} if centred else {})}
        workspace = torch.empty(cabi_x.norm_workspace_bytes(ROWS, width), dtype=torch.uint8, device=DEV)
        state = {bits: forward(xd, rd, gamma, *beta, EPS, p, bits, SEED, y=y, h=h, rstd=rstd)[3] for bits in BITS}
        for bits in BITS:
            arms[f'forward_{bits}'] = (lambda bits=bits: forward(xd, rd, gamma, *beta, EPS, p, bits, SEED, y=y, h=h, rstd=rstd, state=state[bits]), 2 * args.reps)
            arms[f'backward_{bits}'] = (lambda bits=bits: backward(gy, state[bits], rstd, gamma, bits, SEED, p, gh if prenorm else None, dres=dres, dbranch=dbranch,
                                                                   workspace=workspace, **sums), 2 * args.reps)
        runs = {name: [] for name in arms}
        for f, _ in arms.values():                                   # every arm once before any is timed: allocator, code objects, clocks
            timed(f, reps=10, rounds=1)
        for _ in range(2):
            for name, (f, reps) in arms.items():
                runs[name].append(round(timed(f, reps=reps), 2))
        us = {name: min(v) for name, v in runs.items()}
        kernels = {}
        for bits in BITS:
            kept = cabi_x.norm_state_bytes(ROWS, width, bits) + 4 * ROWS
            moved_f = (3 + prenorm) * size * n + kept                 # x + residual + y (+ h) + state + rstd
            moved_b = (2 + prenorm + mask) * size * n + kept          # gy (+ gh) + dres (+ dbranch) + state + rstd
            kernels[str(bits)] = {'forward_bytes_moved': moved_f, 'backward_bytes_moved': moved_b, 'forward_us': us[f'forward_{bits}'],
                                  'backward_us': us[f'backward_{bits}'],
                                  'forward_fraction_of_floor': round(moved_f / PEAK_BYTES_PER_US / us[f'forward_{bits}'], 3),
                                  'backward_fraction_of_floor': round(moved_b / PEAK_BYTES_PER_US / us[f'backward_{bits}'], 3)}
        row = {'rows': ROWS, 'width': width, 'dtype': str(dtype).replace('torch.', ''), 'norm': 'layer_norm' if centred else 'rms_norm', 'p': p, 'prenorm': prenorm,
               'us_forward_plus_backward': {name: us[name] for name in calls}, 'runs_us': runs,
               'fused_over_composed': {str(bits): round(us[f'fused_{bits}'] / us[f'composed_{bits}'], 4) for bits in BITS},
               'fused_over_torch': {str(bits): round(us[f'fused_{bits}'] / us['torch'], 4) for bits in BITS},
               'saved_for_backward_bytes': {name: saved_bytes(f) for name, f in calls.items()}, 'input_bytes': size * n, 'kernels': kernels}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del arms, calls, x, res, gy, gh, xd, rd, y, h, dres, dbranch, state, workspace, leaves
        torch.cuda.empty_cache()
    record = {'what': 'python tools/add_norm_bench.py: fewbit.DropoutAddLayerNorm / DropoutAddRMSNorm forward + backward beside dropout_add + the quantized norm '
                      'and beside torch, and the fused entry points alone; every arm in one process, alternating; us per call',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
