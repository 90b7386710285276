#!/usr/bin/env python3
"""Digests of what the quantized autograd nodes compute and keep, the Python-side sibling of tools/isa_digest.py: after ``torch.manual_seed`` every
case runs forward + backward through one public function and prints one line with the sha256 (first 16 hex digits) of every output, of every
gradient, of every tensor saved for backward (dtype, shape and bytes, seen through ``torch.autograd.graph.saved_tensors_hooks``) and of the host
generator's state afterwards.  Two trees whose listings agree compute, keep and draw the same bytes: how a clean-up of the nodes is shown to
change nothing.  Only public names and ``linear.use_native_sketch`` are used, so one file runs on both trees.

    python3 tools/node_digest.py host > host.txt          # host tensors (fp32, fp16, bf16, float64); no GPU needed
    python3 tools/node_digest.py gpu > gpu.txt            # GPU tensors on the kernels, and with use_native_sketch(False); one process
    diff old.txt new.txt

Cases: linear_quantized; glu_quantized in both forms; gated_mlp_quantized with biases, without, with gate_weight frozen and with only down_bias
trainable; layer_norm_quantized; rms_norm_quantized; the two dropout_add_*_norm_quantized at p = 0 and 0.25, with and without prenorm -- at 2, 4
and 8 bits, 1 and 37 rows, widths 37 (no whole block), 72 and 200 (whole blocks, no whole group) and 256 (the masked fused norms: 72, 200 and
256), plus one bf16-autocast case per function.  A case that raises prints the exception instead: that line has to agree as well.
"""
import hashlib
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import fewbit_amd as fewbit  # noqa: E402
from fewbit_amd import linear  # noqa: E402

FN = fewbit.functional
HIDDEN_OUT = 24


def sha(*parts) -> str:
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else str(p).encode())
    return h.hexdigest()[:16]


def tensor_bytes(t) -> bytes:
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view(torch.uint8).numpy().tobytes()


def of(tensors) -> str:
    return sha(*(part for t in tensors for part in (('none', ) if t is None else (t.dtype, tuple(t.shape), tensor_bytes(t)))))


def leaves(gen, device, dtype, *shapes, grad=True):
    return [None if s is None else torch.randn(s, generator=gen).to(device=device, dtype=dtype).requires_grad_(grad) for s in shapes]


def linear_case(gen, device, dtype, rows, width, bits):
    x, w, b = leaves(gen, device, dtype, (1, rows, width), (HIDDEN_OUT, width), (HIDDEN_OUT, ))
    return (x, w, b), lambda: FN.linear_quantized(x, w, b, bits)


def glu_case(packed):
    def build(gen, device, dtype, rows, width, bits):
        if packed:
            both, = leaves(gen, device, dtype, (1, rows, 2 * width))
            return (both, ), lambda: FN.glu_quantized(both, None, 'silu', bits)
        gate, up = leaves(gen, device, dtype, (1, rows, width), (1, rows, width))
        return (gate, up), lambda: FN.glu_quantized(gate, up, 'gelu', bits)
    return build


def gated_mlp_case(variant):
    def build(gen, device, dtype, rows, width, bits):
        biased = variant != 'nobias'
        x, wg, wu, wd = leaves(gen, device, dtype, (1, rows, width), (width, width), (width, width), (HIDDEN_OUT, width))
        bg, bu, bd = leaves(gen, device, dtype, *(((width, ), (width, ), (HIDDEN_OUT, )) if biased else (None, None, None)))
        if variant == 'frozen_gate':
            wg.requires_grad_(False)
        if variant == 'down_bias_only':
            for t in (x, wg, wu, wd, bg, bu):
                t.requires_grad_(False)
        return (x, wg, wu, wd, bg, bu, bd), lambda: FN.gated_mlp_quantized(x, wg, wu, wd, bg, bu, bd, 'silu', bits)
    return build


def norm_case(centred):
    def build(gen, device, dtype, rows, width, bits):
        x, w, b = leaves(gen, device, dtype, (1, rows, width), (width, ), (width, ))
        if centred:
            return (x, w, b), lambda: FN.layer_norm_quantized(x, (width, ), w, b, 1e-5, bits)
        return (x, w), lambda: FN.rms_norm_quantized(x, (width, ), w, 1e-6, bits)
    return build


def add_norm_case(centred, p, prenorm):
    def build(gen, device, dtype, rows, width, bits):
        x, r, w, b = leaves(gen, device, dtype, (1, rows, width), (1, rows, width), (width, ), (width, ))
        if centred:
            return (x, r, w, b), lambda: FN.dropout_add_layer_norm_quantized(x, r, (width, ), w, b, 1e-5, p, True, bits, prenorm)
        return (x, r, w), lambda: FN.dropout_add_rms_norm_quantized(x, r, (width, ), w, 1e-6, p, True, bits, prenorm)
    return build


CASES = [('linear', linear_case), ('glu_two', glu_case(False)), ('glu_packed', glu_case(True))]
CASES += [(f'gated_mlp_{v}', gated_mlp_case(v)) for v in ('biases', 'nobias', 'frozen_gate', 'down_bias_only')]
CASES += [('layer_norm', norm_case(True)), ('rms_norm', norm_case(False))]
CASES += [(f'add_{"layer" if c else "rms"}_norm_p{p}_{"prenorm" if pre else "postnorm"}', add_norm_case(c, p, pre))
          for c in (True, False) for p in (0.0, 0.25) for pre in (False, True)]


def run(name, build, device, dtype, rows, width, bits, autocast=False) -> str:
    gen = torch.Generator().manual_seed(1000 * rows + width + bits)
    inputs, call = build(gen, device, dtype, rows, width, bits)
    saved = []

    def pack(t):
        saved.append(t)
        return t
    torch.manual_seed(4321)
    try:
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            if autocast:
                with torch.autocast(device, dtype=torch.bfloat16):
                    out = call()
            else:
                out = call()
        outs = out if isinstance(out, tuple) else (out, )
        kept = of(saved)                                   # (digested before backward: what the forward left behind)
        torch.autograd.backward(outs, [torch.randn(o.shape, generator=gen).to(device=device, dtype=o.dtype) for o in outs])
        grads = [None if t is None else t.grad for t in inputs]
        return f'out={of(outs)} grad={of(grads)} saved={len(saved)}:{kept} rng={sha(tensor_bytes(torch.get_rng_state()))}'
    except Exception as e:                                  # noqa: BLE001  (the refusal is part of the behaviour)
        return f'{type(e).__name__}: {str(e)[:120]}'


def listing(device, dtypes, label):
    for name, build in CASES:
        masked = '_p0.25_' in name
        for dtype in dtypes:
            for bits in (2, 4, 8):
                for rows in (1, 37):
                    for width in (72, 200, 256) if masked else (37, 72, 200, 256):
                        print(f'{label} {name} {str(dtype)[6:]} bits={bits} {rows}x{width}: {run(name, build, device, dtype, rows, width, bits)}')
        print(f'{label} {name} autocast-bf16 bits=4 37x72: {run(name, build, device, torch.float32, 37, 72, 4, autocast=True)}')


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else 'host'
    if what == 'host':
        listing('cpu', (torch.float32, torch.float16, torch.bfloat16, torch.float64), 'host')
        return 0
    if not torch.cuda.is_available():
        print('no GPU', file=sys.stderr)
        return 1
    for native in (True, False):
        previous = linear.use_native_sketch(native)
        try:
            listing('cuda', (torch.float32, torch.float16, torch.bfloat16), 'gpu-kernels' if native else 'gpu-pytorch')
        finally:
            linear.use_native_sketch(previous)
    torch.cuda.synchronize()
    return 0


if __name__ == '__main__':
    sys.exit(main())
