"""fewbit.functional.linear_cross_entropy (fewbit_amd/xent.py; the step kernel of fewbit_amd/csrc/fewbit_xent.hip) on MI355X: an LM head and its loss at
16384 tokens, 4096 -> 32000, 4096 -> 128256 and 768 -> 50265 (Llama-2, Llama-3, RoBERTa), bf16 and fp32.  Arms per case, alternating in one process, each
forward + backward (torch.autograd.grad of the mean loss with respect to x and W):
  (a) fewbit.functional.linear_cross_entropy(x, W, t)                         the logits exist one chunk of rows at a time;
  (b) fewbit.functional.cross_entropy(F.linear(x, W), t)                      the logits whole, one float per row beside them;
  (c) the same with inplace_backward=True                                      the gradient written over the logits;
  (d) F.cross_entropy(F.linear(x, W).float(), t)                              the Hugging Face form.
Then (a) at every chunk_rows of a sweep, and on one chunk of logits of the default size, into preallocated outputs:
  (e) cabi_x.cross_entropy_step                                                floor: the chunk once in, once out;
  (f) cabi_x.cross_entropy_forward + cabi_x.cross_entropy_backward in place    the pair that the step replaces: the chunk twice in, once out.
Timing as tools/sketch_bench.py::timed (the GPU kept busy with the same call until it has settled, the median over rounds of back-to-back calls between
HIP events); the arms alternate twice and the smaller median is quoted.  Per arm also the peak of torch's allocator over one forward + backward above what
was allocated before it.  No time is fixed in advance: what is slower is listed as such.

    python tools/linear_cross_entropy_bench.py [--out FILE]        ->  profiles/linear_cross_entropy_bench.json
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
from fewbit_amd import cabi_x, xent
from cross_entropy_bench import peak_bytes
from sketch_bench import timed

DEV = 'cuda'
ROWS = 16384
CASES = tuple((hidden, classes, dtype) for hidden, classes in ((4096, 32000), (4096, 128256), (768, 50265)) for dtype in (torch.bfloat16, torch.float32))
SWEEP = (1024, 2048, 4096, 8192, 16384)
PEAK_BYTES_PER_US = 8.0e6


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'linear_cross_entropy_bench.json'), help='where the record is written')
    ap.add_argument('--reps', type=int, default=3, help='back-to-back calls per timed round of a whole step (the kernels alone: ten times as many)')
    ap.add_argument('--rows', type=int, default=ROWS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    clock = lambda f, reps: round(timed(f, reps=reps, warm=2, settle_s=0.2), 2)
    rows, slower = [], []
    for hidden, classes, dtype in CASES:
        torch.manual_seed(0)
        x = (torch.rand(args.rows, hidden, device=DEV) * 2 - 1).to(dtype).requires_grad_()
        w = ((torch.rand(classes, hidden, device=DEV) * 2 - 1) * 4 / hidden**0.5).to(dtype).requires_grad_()
        t = torch.randint(0, classes, (args.rows, ), device=DEV)
        forwards = {'linear_cross_entropy': lambda: fewbit.functional.linear_cross_entropy(x, w, t),
                    'fewbit': lambda: fewbit.functional.cross_entropy(F.linear(x, w), t),
                    'fewbit_inplace': lambda: fewbit.functional.cross_entropy(F.linear(x, w), t, inplace_backward=True),
                    'torch_float': lambda: F.cross_entropy(F.linear(x, w).float(), t)}
        arms = {name: (lambda forward=forward: torch.autograd.grad(forward(), (x, w))) for name, forward in forwards.items()}
        for f in arms.values():                                        # every arm once before any is timed: allocator, code objects, GEMM plans
            f()
        runs = {name: [] for name in arms}
        for _ in range(2):
            for name, f in arms.items():
                runs[name].append(clock(f, args.reps))
        us = {name: min(v) for name, v in runs.items()}
        for other in ('fewbit', 'fewbit_inplace', 'torch_float'):
            if us['linear_cross_entropy'] > us[other]:
                slower.append(f'{hidden} -> {classes} {dtype}: {us["linear_cross_entropy"]} us against {us[other]} us of {other}')
        peaks = {name: peak_bytes(f) for name, f in arms.items()}
        default = xent.default_chunk_rows(args.rows, hidden, classes)
        sweep = {}
        for chunk in SWEEP:
            f = lambda: torch.autograd.grad(fewbit.functional.linear_cross_entropy(x, w, t, chunk_rows=chunk), (x, w))
            f()
            sweep[chunk] = {'us': clock(f, args.reps), 'peak_allocated_bytes': peak_bytes(f)}
        # the kernels alone on one chunk (the step reads its own output from the second call on: the time does not depend on the values)
        logits = F.linear(x.detach()[:default], w.detach())
        tc, grow = t[:default], torch.full((1, ), 1.0 / args.rows, device=DEV)
        lse, loss = cabi_x.cross_entropy_forward(logits, tc)
        chunk_bytes = logits.numel() * logits.element_size()
        floor = 2 * chunk_bytes / PEAK_BYTES_PER_US
        step = lambda: cabi_x.cross_entropy_step(logits, tc, grow, lse=lse, loss=loss)

        def pair():
            cabi_x.cross_entropy_forward(logits, tc, lse=lse, loss=loss)
            cabi_x.cross_entropy_backward(logits, tc, lse, grow, out=logits)

        alone = {'step': [], 'pair': []}
        for _ in range(2):
            alone['step'].append(clock(step, 10 * args.reps))
            alone['pair'].append(clock(pair, 10 * args.reps))
        kernels = {name: {'us': min(v), 'runs_us': v, 'fraction_of_floor': round(floor / min(v), 3), 'TB_per_s': round(floor / min(v) * 8.0, 3)} for name, v in alone.items()}
        size = x.element_size()
        staged = [b for b in cabi_x.CROSS_ENTROPY_STEP_STAGED_BYTES if classes * size <= b]
        logits_bytes = size * args.rows * classes
        row = {'rows': args.rows, 'hidden': hidden, 'classes': classes, 'dtype': str(dtype).replace('torch.', ''), 'logits_bytes': logits_bytes,
               'weight_bytes': size * classes * hidden, 'default_chunk_rows': default, 'us_forward_plus_backward': us, 'runs_us': runs,
               'over': {other: round(us['linear_cross_entropy'] / us[other], 4) for other in ('fewbit', 'fewbit_inplace', 'torch_float')},
               'peak_allocated_bytes_over_one_step': peaks, 'peak_over_logits': {name: round(v / logits_bytes, 4) for name, v in peaks.items()},
               'chunk_rows_sweep': sweep,
               'step_alone': {'chunk_rows': default, 'chunk_bytes': chunk_bytes, 'byte_floor_us_at_8TBs_one_read_one_write': round(floor, 2),
                              'row_bytes': classes * size, 'variant': f'staged in {staged[0]} bytes of LDS' if staged else 'beyond the tiers: forward + backward in place', **kernels,
                              'step_over_pair': round(kernels['step']['us'] / kernels['pair']['us'], 4)}}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del arms, forwards, x, w, logits
        torch.cuda.empty_cache()
    record = {'what': 'python tools/linear_cross_entropy_bench.py: an LM head and its loss forward + backward (gradients of x and W), chunked against whole '
                      'logits, every arm in one process, alternating; a chunk_rows sweep; the step kernel alone beside the pair it replaces; us per call',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'slower': slower, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    print('slower:', slower or 'none')


if __name__ == '__main__':
    main()
