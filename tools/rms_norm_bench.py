"""QuantizedRMSNorm (fewbit_amd/norm.py, fewbit_amd/csrc/fewbit_norm.hip) on MI355X at 16384 rows of 768, 3072 and 4096 elements (the Llama width: two
blocks per forward lane, 512 lanes per backward row), bf16 and fp32.  Arms per case, alternating in one process, each forward + backward
(torch.autograd.grad of the input and gamma on a random gradient):
  (a) torch.nn.RMSNorm                                              keeps its input (and what its backward needs besides);
  (b) fewbit.QuantizedRMSNorm(bits=2 / 4 / 8)                       keeps the normalized rows in a few bits and rstd;
and the entry points alone, into preallocated outputs, for their share of the byte floor at 8 TB/s:
  (c) cabi_x.rms_norm_forward                                       floor: x + y + state + rstd bytes;
  (d) cabi_x.rms_norm_backward (both launches)                      floor: gy + state + rstd + dx bytes;
  (e) cabi_x.layer_norm_forward / layer_norm_backward               the centred kernels on the same tensors: the un-centred ones do strictly less
                                                                    and must not take longer (2 % margin, the box-to-box spread);
  (f) with --parent-lib FILE, the layer-norm entry points of that build of libfewbit_hipx.so (the parent commit's), called through ctypes.
Timing as tools/sketch_bench.py::timed: the GPU is kept busy with the same call until it has settled, then the median over rounds of many
back-to-back calls between HIP events; the arms alternate twice and the smaller median is quoted.  Bytes saved for backward are counted with
fewbit.memory_usage_hooks (gamma included, which every arm keeps).  Beside each quantized arm: the relative error of one input gradient and
of one gamma gradient against float64.

    python tools/rms_norm_bench.py [--out FILE] [--parent-lib FILE]        ->  profiles/rms_norm_bench.json
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # tools/ -> repository root
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch
import fewbit_amd as fewbit
from fewbit_amd import cabi_x
from fewbit_amd.cabi import DTYPES
from sketch_bench import timed

DEV = 'cuda'
ROWS, SEED, EPS = 16384, 2026, 1e-5
CASES = tuple((width, dtype) for width in (768, 3072, 4096) for dtype in (torch.bfloat16, torch.float32))
BITS = (2, 4, 8)
PEAK_BYTES_PER_US = 8.0e6
MARGIN = 1.02


def saved_bytes(f):
    with fewbit.memory_usage_hooks() as usage:
        f()
    return usage.forward or 0


def parent_entry_points(path):
    """the layer-norm entry points of another build of the companion library -> (forward, backward) taking the tensors of the arms below"""
    L = ctypes.CDLL(path)
    vp, sz, i32, dbl, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double, ctypes.c_uint64
    L.fewbit_hipx_layer_norm_forward.restype = L.fewbit_hipx_layer_norm_backward.restype = i32
    L.fewbit_hipx_layer_norm_forward.argtypes = [i32, vp, sz, sz, vp, vp, dbl, i32, u64, vp, vp, vp, vp, sz, vp, vp]
    L.fewbit_hipx_layer_norm_backward.argtypes = [i32, vp, vp, vp, vp, sz, sz, i32, vp, vp, vp, vp, sz, vp]
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def forward(x, gamma, beta, bits, y, rstd, state):
        assert L.fewbit_hipx_layer_norm_forward(DTYPES[x.dtype], x.data_ptr(), x.shape[0], x.shape[1], gamma.data_ptr(), beta.data_ptr(), EPS, bits, SEED, None,
                                                y.data_ptr(), rstd.data_ptr(), state.data_ptr(), state.numel(), None, stream()) == 0

    def backward(gy, state, rstd, gamma, bits, dx, dgamma, dbeta, workspace):
        assert L.fewbit_hipx_layer_norm_backward(DTYPES[gy.dtype], gy.data_ptr(), state.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), gy.shape[0], gy.shape[1], bits,
                                                 dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), workspace.data_ptr(), workspace.numel(), stream()) == 0

    return forward, backward


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rms_norm_bench.json'), help='where the record is written')
    ap.add_argument('--reps', type=int, default=50, help='back-to-back calls per timed round')
    ap.add_argument('--parent-lib', default=None, help="a libfewbit_hipx.so of the parent commit: its layer-norm entry points are timed as well")
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    parent = parent_entry_points(args.parent_lib) if args.parent_lib else None
    rows, slower = [], []
    for width, dtype in CASES:
        torch.manual_seed(0)
        x = (3 + 2 * torch.randn(ROWS, width, device=DEV)).to(dtype).requires_grad_()
        gy = torch.randn(ROWS, width, device=DEV).to(dtype)
        layers = {'nn_rms_norm': torch.nn.RMSNorm(width, eps=EPS, device=DEV, dtype=dtype)}
        with torch.no_grad():
            layers['nn_rms_norm'].weight.copy_(1 + 0.5 * torch.randn(width, device=DEV))
        for bits in BITS:
            layers[f'quantized_{bits}'] = fewbit.QuantizedRMSNorm.from_rms_norm(layers['nn_rms_norm'], bits=bits)
        step = lambda layer: torch.autograd.grad(layer(x), (x, layer.weight), gy)
        arms = {name: (lambda layer=layer: step(layer), args.reps) for name, layer in layers.items()}
        n, size, xd = ROWS * width, x.element_size(), x.detach()
        gamma = layers['nn_rms_norm'].weight.detach()
        beta = torch.randn(width, device=DEV).to(dtype)
        y, dx, rstd = torch.empty_like(xd), torch.empty_like(xd), torch.empty(ROWS, dtype=torch.float32, device=DEV)
        dgamma, dbeta = torch.empty(width, dtype=torch.float32, device=DEV), torch.empty(width, dtype=torch.float32, device=DEV)
        workspace = torch.empty(cabi_x.norm_workspace_bytes(ROWS, width), dtype=torch.uint8, device=DEV)
        state = {bits: cabi_x.rms_norm_forward(xd, gamma, EPS, bits, SEED, y=y, rstd=rstd)[2] for bits in BITS}
        for bits in BITS:
            arms[f'forward_{bits}'] = (lambda bits=bits: cabi_x.rms_norm_forward(xd, gamma, EPS, bits, SEED, y=y, rstd=rstd, state=state[bits]), 2 * args.reps)
            arms[f'backward_{bits}'] = (lambda bits=bits: cabi_x.rms_norm_backward(gy, state[bits], rstd, gamma, bits, dx=dx, dgamma=dgamma, workspace=workspace),
                                        2 * args.reps)
            arms[f'layer_norm_forward_{bits}'] = (lambda bits=bits: cabi_x.layer_norm_forward(xd, gamma, beta, EPS, bits, SEED, y=y, rstd=rstd, state=state[bits]),
                                                  2 * args.reps)
            arms[f'layer_norm_backward_{bits}'] = (lambda bits=bits: cabi_x.layer_norm_backward(gy, state[bits], rstd, gamma, bits, dx=dx, dgamma=dgamma, dbeta=dbeta,
                                                                                                 workspace=workspace), 2 * args.reps)
            if parent is not None:
                arms[f'parent_layer_norm_forward_{bits}'] = (lambda bits=bits: parent[0](xd, gamma, beta, bits, y, rstd, state[bits]), 2 * args.reps)
                arms[f'parent_layer_norm_backward_{bits}'] = (lambda bits=bits: parent[1](gy, state[bits], rstd, gamma, bits, dx, dgamma, dbeta, workspace),
                                                              2 * args.reps)
        arms['forward_plain'] = (lambda: cabi_x.rms_norm_forward(xd, gamma, EPS, keep=False, y=y, rstd=rstd), 2 * args.reps)
        runs = {name: [] for name in arms}
        for f, _ in arms.values():                                   # every arm once before any is timed: allocator, code objects, clocks
            timed(f, reps=10, rounds=1)
        for _ in range(2):
            for name, (f, reps) in arms.items():
                runs[name].append(round(timed(f, reps=reps), 2))
        us = {name: min(v) for name, v in runs.items()}
        for bits in BITS:                                            # (the states hold layer-norm rows after those arms: the RMS ones again for the errors)
            cabi_x.rms_norm_forward(xd, gamma, EPS, bits, SEED, y=y, rstd=rstd, state=state[bits])
        x64 = xd.double().requires_grad_()
        (exact, ) = torch.autograd.grad(torch.nn.functional.rms_norm(x64, (width, ), gamma.double(), EPS), x64, gy.double())
        x64 = x64.detach()
        xhat = x64 / torch.sqrt(x64.square().mean(dim=1, keepdim=True) + EPS)
        exact_gamma = (gy.double() * xhat).sum(dim=0)
        error = {}
        for name, layer in layers.items():
            gx, gw = step(layer)
            error[name] = {'input_gradient': round(float((gx.double() - exact).norm() / exact.norm()), 5),
                           'gamma_gradient': round(float((gw.double() - exact_gamma).norm() / exact_gamma.norm()), 5)}
        kernels = {}
        for bits in BITS:
            kept = cabi_x.norm_state_bytes(ROWS, width, bits)
            moved = 2 * size * n + kept + 4 * ROWS                   # forward: x + y + state + rstd; backward: gy + state + rstd + dx
            floor = moved / PEAK_BYTES_PER_US
            centred = {d: us[f'layer_norm_{d}_{bits}'] for d in ('forward', 'backward')}
            if parent is not None:
                centred = {d: min(centred[d], us[f'parent_layer_norm_{d}_{bits}']) for d in centred}
            kernels[str(bits)] = {'bytes_moved': moved, 'byte_floor_us_at_8TBs': round(floor, 2), 'forward_us': us[f'forward_{bits}'], 'backward_us': us[f'backward_{bits}'],
                                  'forward_fraction_of_floor': round(floor / us[f'forward_{bits}'], 3),
                                  'backward_fraction_of_floor': round(floor / us[f'backward_{bits}'], 3),
                                  'layer_norm_forward_us': us[f'layer_norm_forward_{bits}'], 'layer_norm_backward_us': us[f'layer_norm_backward_{bits}'],
                                  'forward_over_layer_norm': round(us[f'forward_{bits}'] / centred['forward'], 4),
                                  'backward_over_layer_norm': round(us[f'backward_{bits}'] / centred['backward'], 4)}
            if parent is not None:
                kernels[str(bits)].update(parent_layer_norm_forward_us=us[f'parent_layer_norm_forward_{bits}'],
                                          parent_layer_norm_backward_us=us[f'parent_layer_norm_backward_{bits}'])
            for d in ('forward', 'backward'):
                if width in (768, 3072) and us[f'{d}_{bits}'] > MARGIN * centred[d]:
                    slower.append(f'{width} {dtype} bits {bits} {d}: {us[f"{d}_{bits}"]} us against {centred[d]} us of the layer norm')
        row = {'rows': ROWS, 'width': width, 'dtype': str(dtype).replace('torch.', ''),
               'us_forward_plus_backward': {name: us[name] for name in layers}, 'runs_us': runs,
               'over_nn_rms_norm': {name: round(us[name] / us['nn_rms_norm'], 4) for name in layers},
               'saved_for_backward_bytes': {name: saved_bytes(lambda layer=layer: layer(x)) for name, layer in layers.items()},
               'input_bytes': size * n, 'kept_of_the_input_bytes': {str(bits): cabi_x.norm_state_bytes(ROWS, width, bits) + 4 * ROWS for bits in BITS},
               'plain_forward_us': us['forward_plain'], 'relative_error_of_one_call': error, 'kernels': kernels}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del arms, layers, x, gy, xd, y, dx, state, workspace, exact, x64, xhat
        torch.cuda.empty_cache()
    record = {'what': 'python tools/rms_norm_bench.py: QuantizedRMSNorm forward + backward beside nn.RMSNorm, the forward and backward entry points alone, '
                      'and the layer-norm entry points on the same tensors; every arm in one process, alternating; us per call',
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'parent_library_timed': parent is not None,
              'slower_than_the_layer_norm_by_more_than_2_percent': slower, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    print('slower than the layer norm by more than 2 %:', slower or 'none')


if __name__ == '__main__':
    main()
