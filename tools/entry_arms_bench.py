#!/usr/bin/env python3
"""The entry-point arms of tools/quant_linear_bench.py (pack_*, unpack_*), dropout_bench.py (kernel, kernel_add), glu_bench.py (forward_*, backward_*,
forward_plain) and layer_norm_bench.py (the same three) at the smallest size of each tool, bf16 and fp32, and nothing else of those tools: the arms
whose time is one launch into preallocated buffers, so the ones a change of the C host code in front of a launch can move.  Built and timed as the
tools do (tools/sketch_bench.py::timed, every arm once before any is timed, two alternations, the smaller median quoted).  `--root` names the tree
whose package and library are measured, so one file measures a checkout of another commit beside this one; `--rows` (default: the tools' 16384)
makes the kernels short enough for the launch itself to be the whole arm.  `--families core` / `companion` times only the four activation entry points
of libfewbit_hip.so (quantize_forward with gelu and 15 borders, quantize_backward, stepwise1_forward and stepwise1_backward with relu, through
fewbit_amd.cabi's pre-resolved launches, at rows x 768 and at n = 4096, where the arm is bound by the launch) or only the arms of the companion library.

    python tools/entry_arms_bench.py [--root TREE] [--rows N]        ->  one JSON line: {"root", "rows", "us": {arm: microseconds}}
"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--rows', type=int, default=16384)
ap.add_argument('--reps', type=int, default=200, help='back-to-back calls per timed round')
ap.add_argument('--families', choices=('all', 'core', 'companion'), default='all')
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch  # noqa: E402
from fewbit_amd import cabi, cabi_x  # noqa: E402
from sketch_bench import timed  # noqa: E402

DEV, SEED, P, EPS, BITS = 'cuda', 2026, 0.1, 1e-5, (2, 4, 8)
ROWS = args.rows


def core_arms_of(dtype):
    """the four activation entry points of libfewbit_hip.so, each one launch into preallocated buffers"""
    tag = str(dtype).replace('torch.', '')
    borders = torch.linspace(-3, 3, 15, device=DEV).to(dtype)
    levels = torch.linspace(0, 1, 16, device=DEV).to(dtype)
    arms = {}
    for n in (ROWS * 768, 4096):
        x, gy = torch.randn(n, device=DEV).to(dtype), torch.randn(n, device=DEV).to(dtype)
        y, gx = torch.empty_like(x), torch.empty_like(x)
        state, bit = (torch.empty(cabi.state_nbytes(n, k), dtype=torch.uint8, device=DEV) for k in (4, 1))
        arms[f'core {tag} quantize_forward n={n}'] = cabi.bind_forward('gelu', x, borders, y, state)
        arms[f'core {tag} quantize_backward n={n}'] = cabi.bind_backward(gy, state, levels, gx)
        arms[f'core {tag} stepwise1_forward n={n}'] = cabi.bind_stepwise1_forward('relu', x, y, bit)
        arms[f'core {tag} stepwise1_backward n={n}'] = cabi.bind_stepwise1_backward('relu', gy, bit, gx)
    return arms


def arms_of(dtype):
    tag = str(dtype).replace('torch.', '')
    new = lambda width: torch.randn(ROWS, width, device=DEV).to(dtype)
    arms = core_arms_of(dtype) if args.families != 'companion' else {}
    if args.families == 'core':
        return arms
    # quant_linear_bench: 16384 x 768
    x, n = new(768), ROWS * 768
    out, packed = torch.empty_like(x), {bits: cabi_x.quant_pack(x, SEED, bits) for bits in BITS}
    for bits in BITS:
        arms[f'quant {tag} pack_{bits}'] = lambda bits=bits: cabi_x.quant_pack(x, SEED, bits, out=packed[bits])
        arms[f'quant {tag} unpack_{bits}'] = lambda bits=bits: cabi_x.quant_unpack(packed[bits], n, bits, dtype, out=out)
    # dropout_bench: 16384 x 768
    r, dropped = new(768), torch.empty_like(x)
    arms[f'dropout {tag} kernel'] = lambda: cabi_x.dropout_apply(x, SEED, P, out=dropped)
    arms[f'dropout {tag} kernel_add'] = lambda: cabi_x.dropout_apply(x, SEED, P, r, out=dropped)
    # layer_norm_bench: 16384 x 768
    gamma, beta, gy = (1 + 0.5 * torch.randn(768, device=DEV)).to(dtype), torch.randn(768, device=DEV).to(dtype), new(768)
    y, dx, rstd = torch.empty_like(x), torch.empty_like(x), torch.empty(ROWS, dtype=torch.float32, device=DEV)
    dgamma, dbeta = torch.empty(768, dtype=torch.float32, device=DEV), torch.empty(768, dtype=torch.float32, device=DEV)
    workspace = torch.empty(cabi_x.norm_workspace_bytes(ROWS, 768), dtype=torch.uint8, device=DEV)
    norm_state = {bits: cabi_x.layer_norm_forward(x, gamma, beta, EPS, bits, SEED, y=y, rstd=rstd)[2] for bits in BITS}
    for bits in BITS:
        arms[f'layer_norm {tag} forward_{bits}'] = lambda bits=bits: cabi_x.layer_norm_forward(x, gamma, beta, EPS, bits, SEED, y=y, rstd=rstd, state=norm_state[bits])
        arms[f'layer_norm {tag} backward_{bits}'] = lambda bits=bits: cabi_x.layer_norm_backward(gy, norm_state[bits], rstd, gamma, bits, dx=dx, dgamma=dgamma, dbeta=dbeta,
                                                                                                 workspace=workspace)
    arms[f'layer_norm {tag} forward_plain'] = lambda: cabi_x.layer_norm_forward(x, gamma, beta, EPS, keep=False, y=y, rstd=rstd)
    # glu_bench: 16384 x 3072
    gate, up, g_y = new(3072), new(3072), new(3072)
    product, d_gate, d_up = torch.empty_like(gate), torch.empty_like(gate), torch.empty_like(gate)
    glu_state = {bits: cabi_x.glu_forward(gate, up, 'silu', bits, SEED, y=product)[1] for bits in BITS}
    for bits in BITS:
        arms[f'glu {tag} forward_{bits}'] = lambda bits=bits: cabi_x.glu_forward(gate, up, 'silu', bits, SEED, y=product, state=glu_state[bits])
        arms[f'glu {tag} backward_{bits}'] = lambda bits=bits: cabi_x.glu_backward(g_y, glu_state[bits], 'silu', bits, d_gate=d_gate, d_up=d_up)
    arms[f'glu {tag} forward_plain'] = lambda: cabi_x.glu_forward(gate, up, 'silu', keep=False, y=product)
    return arms


def main():
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    us = {}
    for dtype in (torch.bfloat16, torch.float32):
        arms = arms_of(dtype)
        runs = {name: [] for name in arms}
        for f in arms.values():                                      # every arm once before any is timed: allocator, code objects, clocks
            timed(f, reps=10, rounds=1)
        for _ in range(2):
            for name, f in arms.items():
                runs[name].append(round(timed(f, reps=args.reps), 2))
        us.update({name: min(v) for name, v in runs.items()})
    print(json.dumps({'root': os.path.relpath(ROOT), 'rows': ROWS, 'library': os.path.relpath(cabi_x.LIB_PATH), 'us': us}))


if __name__ == '__main__':
    main()
