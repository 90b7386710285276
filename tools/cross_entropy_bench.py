"""fewbit.functional.cross_entropy (fewbit_amd/xent.py, fewbit_amd/csrc/fewbit_xent.hip) on MI355X at 16384 rows of 32000, 50265 and 128256 classes
(Llama-2, RoBERTa, Llama-3), bf16 and fp32.  Arms per case, alternating in one process, each forward + backward (torch.autograd.grad of the mean
loss with respect to the logits):
  (a) fewbit.functional.cross_entropy(x, t)                         keeps x itself and one float per row;
  (b) the same with inplace_backward=True                           the gradient is written over the logits (its own copy of x: the values it
                                                                    reads from the second call on are gradients; the time does not depend on them);
  (c) F.cross_entropy(x, t)                                         keeps the log-softmax in the dtype of x;
  (d) F.cross_entropy(x.float(), t)                                 the Hugging Face form: an fp32 copy, the fp32 log-softmax, an fp32 gradient and its cast;
  (e) F.cross_entropy(x, t) under torch.autocast(bfloat16)          torch runs it in fp32: the same;
and the entry points alone, into preallocated outputs, for their share of the byte floor at 8 TB/s:
  (f) cabi_x.cross_entropy_forward                                  floor: the logits once;
  (g) cabi_x.cross_entropy_backward                                 floor: the logits once, the gradient once;
  (h) the same in place.
Timing as tools/sketch_bench.py::timed: the GPU is kept busy with the same call until it has settled, then the median over rounds of many
back-to-back calls between HIP events; the arms alternate twice and the smaller median is quoted.  Per arm also: the bytes autograd saves
(fewbit.memory_usage_hooks, which counts a tensor that two nodes save twice), the bytes of the distinct storages that keeps alive and how many of
them are not the logits' own storage, and the peak of torch's allocator over one forward + backward above
what was allocated before it.  No time is fixed in advance: what is slower than torch is listed as such.

    python tools/cross_entropy_bench.py [--out FILE]        ->  profiles/cross_entropy_bench.json
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
ROWS = 16384
CASES = tuple((width, dtype) for width in (32000, 50265, 128256) for dtype in (torch.bfloat16, torch.float32))
PEAK_BYTES_PER_US = 8.0e6
TORCH_ARMS = ('torch', 'torch_float', 'torch_autocast')


def saved_bytes(forward, x):
    """(bytes autograd packs in ``forward()`` as ``fewbit.memory_usage_hooks`` counts them: every packed tensor, so a tensor two nodes save counts
    twice; bytes of the distinct storages it keeps alive; those of them that are not the storage of ``x``)"""
    kept = {}

    def pack(t):
        kept[t.untyped_storage().data_ptr()] = t.untyped_storage().nbytes()
        return t

    with fewbit.memory_usage_hooks() as usage:
        forward()
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):          # (a run of its own: only the innermost pair of hooks is applied)
        loss = forward()                                                       # (alive while the storages are told apart by their addresses)
    own = x.untyped_storage().data_ptr()
    del loss
    return usage.forward or 0, sum(kept.values()), sum(n for p, n in kept.items() if p != own)


def peak_bytes(step):
    """the allocator's peak during one ``step()`` above what was allocated before it"""
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def autocast(x, t):
    with torch.autocast('cuda', dtype=torch.bfloat16):
        return F.cross_entropy(x, t)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cross_entropy_bench.json'), help='where the record is written')
    ap.add_argument('--reps', type=int, default=10, help='back-to-back calls per timed round')
    ap.add_argument('--rows', type=int, default=ROWS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    rows, slower = [], []
    for width, dtype in CASES:
        torch.manual_seed(0)
        x = (4.0 * torch.randn(args.rows, width, device=DEV)).to(dtype).requires_grad_()
        own = x.detach().clone().requires_grad_()                      # what the in-place arm overwrites
        t = torch.randint(0, width, (args.rows, ), device=DEV)           # (no ignored row: backward would not read it, and the floors count every logit)
        forwards = {'fewbit': (lambda: fewbit.functional.cross_entropy(x, t), x),
                    'fewbit_inplace': (lambda: fewbit.functional.cross_entropy(own, t, inplace_backward=True), own),
                    'torch': (lambda: F.cross_entropy(x, t), x),
                    'torch_float': (lambda: F.cross_entropy(x.float(), t), x),
                    'torch_autocast': (lambda: autocast(x, t), x)}
        step = lambda forward, leaf: torch.autograd.grad(forward(), leaf)
        arms = {name: (lambda forward=forward, leaf=leaf: step(forward, leaf), args.reps) for name, (forward, leaf) in forwards.items()}
        xd, size = x.detach(), x.element_size()
        lse, loss = cabi_x.cross_entropy_forward(xd, t)
        out, grow, scratch = torch.empty_like(xd), torch.full((1, ), 1.0 / args.rows, device=DEV), xd.clone()
        arms['forward'] = (lambda: cabi_x.cross_entropy_forward(xd, t, lse=lse, loss=loss), 2 * args.reps)
        arms['backward'] = (lambda: cabi_x.cross_entropy_backward(xd, t, lse, grow, out=out), 2 * args.reps)
        arms['backward_inplace'] = (lambda: cabi_x.cross_entropy_backward(scratch, t, lse, grow, out=scratch), 2 * args.reps)
        runs = {name: [] for name in arms}
        for f, _ in arms.values():                                     # every arm once before any is timed: allocator, code objects, clocks
            timed(f, reps=3, rounds=1)
        for _ in range(2):
            for name, (f, reps) in arms.items():
                runs[name].append(round(timed(f, reps=reps), 2))
        us = {name: min(v) for name, v in runs.items()}
        # one gradient of the kernel path against torch's fp32 formulation of the same logits
        want = step(*forwards['torch_float'])[0].float()
        got = step(*forwards['fewbit'])[0].float()
        error = round(float((got - want).norm() / want.norm()), 6)
        del want, got
        logits_bytes = size * args.rows * width
        floors = {'forward': logits_bytes / PEAK_BYTES_PER_US, 'backward': 2 * logits_bytes / PEAK_BYTES_PER_US,
                  'backward_inplace': 2 * logits_bytes / PEAK_BYTES_PER_US}
        kernels = {name: {'us': us[name], 'byte_floor_us_at_8TBs': round(floor, 2), 'fraction_of_floor': round(floor / us[name], 3),
                          'TB_per_s': round(floor / us[name] * 8.0, 3)} for name, floor in floors.items()}
        for name in ('fewbit', 'fewbit_inplace'):
            for other in TORCH_ARMS:
                if us[name] > us[other]:
                    slower.append(f'{width} {dtype} {name}: {us[name]} us against {us[other]} us of {other}')
        saved = {name: saved_bytes(forward, leaf) for name, (forward, leaf) in forwards.items()}
        row = {'rows': args.rows, 'width': width, 'dtype': str(dtype).replace('torch.', ''), 'logits_bytes': logits_bytes,
               'us_forward_plus_backward': {name: us[name] for name in forwards}, 'runs_us': runs,
               'over_torch': {name: {other: round(us[name] / us[other], 4) for other in TORCH_ARMS} for name in ('fewbit', 'fewbit_inplace')},
               'packed_for_backward_bytes': {name: s[0] for name, s in saved.items()},
               'saved_storage_bytes': {name: s[1] for name, s in saved.items()},
               'saved_beyond_the_logits_bytes': {name: s[2] for name, s in saved.items()},
               'saved_over_logits': {name: round(s[1] / logits_bytes, 4) for name, s in saved.items()},
               'peak_allocated_bytes_over_one_step': {name: peak_bytes(arms[name][0]) for name in forwards},
               'relative_error_of_one_gradient_against_torch_float': error, 'kernels': kernels}
        row['peak_over_logits'] = {name: round(v / logits_bytes, 4) for name, v in row['peak_allocated_bytes_over_one_step'].items()}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del arms, forwards, x, own, xd, out, scratch, lse, loss
        torch.cuda.empty_cache()
    record = {'what': 'python tools/cross_entropy_bench.py: fewbit.functional.cross_entropy forward + backward beside F.cross_entropy on the logits as given, '
                      'on their fp32 copy and under autocast, and the forward and backward entry points alone; every arm in one process, alternating; '
                      'us per call',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'slower_than_torch': slower, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    print('slower than torch:', slower or 'none')


if __name__ == '__main__':
    main()
