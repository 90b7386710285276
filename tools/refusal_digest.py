#!/usr/bin/env python3
"""What the entry points of libfewbit_hipx.so refuse, and in which words: the C-side sibling of tools/node_digest.py.  Every entry point of the quant,
glu, norm, fused-norm and dropout families is called through ctypes with each single bad argument in turn and with pairs of bad arguments (which
refusal a call with two faults gets is behaviour), and one line per call gives the status and, where it is not FEWBIT_OK, fewbit_hipx_last_error().
Two trees whose listings agree refuse the same calls in the same order with the same bytes: how a clean-up of the host code is shown to change nothing.

    python3 tools/refusal_digest.py > new.txt             # no GPU needed
    python3 tools/refusal_digest.py --library other/fewbit_amd/libfewbit_hipx.so > old.txt
    diff old.txt new.txt

No call reaches a launch or touches memory, so pointers are plain integers: P is an address aligned to 64 KiB that nobody owns.  To make that certain
and not merely intended, every call carries a *backstop* -- a fault that the entry point tests LAST (a buffer one byte too short, a missing output)
-- unless the case changes that very argument, and then the next backstop of the entry point is taken (or none, where the case says that its own
fault is a refusal for certain).  A call that still got as far as a launch would report "the launch failed" (the process sees no device: HIP_VISIBLE_DEVICES is set to -1 before the library is loaded) and ends the script
with status 1.
"""
import argparse
import ctypes
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
P = 0x10000
KINDS = {'i': ctypes.c_int, 'z': ctypes.c_size_t, 'Q': ctypes.c_uint64, 'u': ctypes.c_uint32, 'p': ctypes.c_void_p, 'd': ctypes.c_double}
F32, F16, BF16 = 0, 1, 2
GELU, SILU = 2, 8
BEYOND = 2**36 + 1
ROWS, WIDTH, N = 5, 200, 1000
ALONE = 'no backstop'      # a case that sets it true is refused by what it names, whatever else: it takes or replaces every backstop


def show(name, value):
    if value is None:
        return f'{name}=NULL'
    if isinstance(value, int) and P <= value < P + 64:
        return f'{name}=P+{value - P}' if value != P else f'{name}=P'
    return f'{name}={value}'


class Entry:
    """one entry point: its signature ('i:dtype p:src ...'), a call that would be valid, and its backstops (see the module's docstring)"""

    def __init__(self, lib, name, signature, base, backstops):
        self.name, self.base, self.backstops = name, base, backstops
        self.args = [part.split(':') for part in signature.split()]
        self.fn = getattr(lib, 'fewbit_hipx_' + name)
        self.fn.restype = ctypes.c_int
        self.fn.argtypes = [KINDS[kind] for kind, _ in self.args]
        missing = [arg for _, arg in self.args if arg not in base]
        assert not missing, (name, missing)

    def call(self, lib, out, bad):
        bad = dict(bad)
        stop = {} if bad.pop(ALONE, False) else next((b for b in self.backstops if not set(b) & set(bad)), None)
        assert stop is not None, f'{self.name}: no backstop is left for {sorted(bad)}'
        values = {**self.base, **stop, **bad}
        status = self.fn(*(values[arg] for _, arg in self.args))
        message = lib.fewbit_hipx_last_error().decode() if status != 0 else ''
        what = ', '.join(show(k, v) for k, v in bad.items()) or 'the backstop alone'
        out.append(f'{self.name} [{what}] -> {status}' + (f' "{message}"' if status != 0 else ''))
        return 'launch' not in message


def cases_of(entry, singles, pairs):
    """singles: {argument: values}; pairs: dicts of two or more bad arguments"""
    for arg, values in singles.items():
        for value in values:
            yield {arg: value}
    yield from pairs
    yield {}


def pointer(*offsets, null=True):
    return ([None] if null else []) + [P + o for o in offsets]


def entries(lib):
    size = lambda name, *a: getattr(lib, 'fewbit_hipx_' + name)(*a)
    for name in ('quant_bytes', 'glu_state_bytes'):
        fn = getattr(lib, 'fewbit_hipx_' + name)
        fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_size_t, ctypes.c_int]
    lib.fewbit_hipx_norm_state_bytes.restype, lib.fewbit_hipx_norm_state_bytes.argtypes = ctypes.c_size_t, [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
    lib.fewbit_hipx_norm_workspace.restype, lib.fewbit_hipx_norm_workspace.argtypes = ctypes.c_size_t, [ctypes.c_size_t, ctypes.c_size_t]
    bits, dtypes, counts, widths = [0, 3, 16], [3, -1], [0, BEYOND], [0, 8193]
    seed_word = pointer(1, 2, 4, null=False)

    # ---- the packed form of a seed ----
    host = dict(n=N, bits=4, seed=7)
    yield Entry(lib, 'quant_pack_host', 'p:x_host z:n i:bits Q:seed p:out_host', dict(host, x_host=P, out_host=P), [dict(out_host=None), dict(x_host=None)]), \
        dict(bits=bits, n=counts, x_host=[None], out_host=[None]), [dict(bits=3, n=BEYOND), dict(n=BEYOND, x_host=None), dict(bits=0, x_host=None)]
    yield Entry(lib, 'quant_unpack_host', 'p:packed_host z:n i:bits p:out_host', dict(host, packed_host=P, out_host=P), [dict(out_host=None), dict(packed_host=None)]), \
        dict(bits=bits, n=counts, packed_host=[None], out_host=[None]), [dict(bits=3, n=BEYOND), dict(n=BEYOND, packed_host=None)]
    need = size('quant_bytes', N, 4)
    yield Entry(lib, 'quant_pack', 'i:dtype p:src z:n i:bits Q:seed p:seed_device p:out z:out_bytes p:stream',
                dict(dtype=F32, src=P, n=N, bits=4, seed=7, seed_device=None, out=P, out_bytes=need, stream=None), [dict(out_bytes=need - 1), dict(out=P + 4)]), \
        dict(dtype=dtypes, bits=bits, n=counts, seed_device=seed_word, src=pointer(1, 2, 4, 8), out=pointer(1, 2, 4, 8)), \
        [dict(dtype=3, bits=3), dict(bits=3, seed_device=P + 4), dict(seed_device=P + 4, n=BEYOND), dict(n=BEYOND, src=None), dict(src=P + 1, out=P + 1),
         {'out': P + 4, 'out_bytes': 0, ALONE: True}, {'out_bytes': 0, ALONE: True}, dict(dtype=BF16, src=P + 1), dict(dtype=BF16, src=P + 2), dict(dtype=F16, src=P + 1), dict(n=0, src=None)]
    yield Entry(lib, 'quant_unpack', 'p:packed z:n i:bits i:out_dtype p:out p:stream', dict(packed=P, n=N, bits=4, out_dtype=F32, out=P, stream=None),
                [dict(out=P + 1), dict(packed=P + 4)]), \
        dict(out_dtype=dtypes, bits=bits, n=counts, packed=pointer(1, 2, 4, 8), out=pointer(1, 2, 4, 8)), \
        [dict(out_dtype=3, bits=3), dict(bits=3, n=BEYOND), dict(n=BEYOND, packed=None), {'packed': P + 4, 'out': P + 2, ALONE: True}, dict(out_dtype=BF16, out=P + 1),
         {'out_dtype': BF16, 'out': P + 2, 'packed': P + 1, ALONE: True}]

    # ---- the gate and the up of a seed ----
    yield Entry(lib, 'glu_state_host', 'p:gate_host p:up_host z:n i:bits Q:seed p:out_host', dict(host, gate_host=P, up_host=P, out_host=P),
                [dict(out_host=None), dict(gate_host=None)]), \
        dict(bits=bits, n=counts, gate_host=[None], up_host=[None], out_host=[None]), [dict(bits=3, n=BEYOND), dict(n=BEYOND, up_host=None)]
    need = size('glu_state_bytes', ROWS * WIDTH, 4)
    shape = dict(dtype=F32, act=SILU, rows=ROWS, width=WIDTH, bits=4, stream=None)
    acts = [0, 3, -1]
    yield Entry(lib, 'glu_forward', 'i:dtype i:act p:gate z:ld_gate p:up z:ld_up z:rows z:width i:bits Q:seed p:seed_device p:y p:state z:state_bytes p:stream',
                dict(shape, gate=P, ld_gate=WIDTH, up=P, ld_up=WIDTH, seed=7, seed_device=None, y=P, state=P, state_bytes=need),
                [dict(state_bytes=need - 1), dict(state=P + 4)]), \
        dict(dtype=dtypes, act=acts, bits=bits, seed_device=seed_word, rows=[0, BEYOND], width=[0, BEYOND], ld_gate=[WIDTH - 1], ld_up=[WIDTH - 1],
             gate=pointer(1, 2, 4, 8), up=pointer(1, 2, 4, 8), y=pointer(1, 2, 4, 8), state=pointer(1, 2, 4, null=False)), \
        [dict(bits=3, seed_device=P + 4), dict(seed_device=P + 4, dtype=3), dict(dtype=3, act=3), dict(act=3, width=0), dict(rows=2**20, width=2**20),
         dict(width=0, ld_gate=0), dict(ld_up=1, gate=None), dict(gate=None, up=P + 1), dict(y=P + 2, state=P + 4), {'state_bytes': 0, ALONE: True}, dict(dtype=BF16, gate=P + 1), dict(dtype=BF16, y=P + 2),
         dict(rows=0, gate=None)]
    backward = dict(shape, gy=P, state=P, d_gate=None, ld_dgate=WIDTH, d_up=None, ld_dup=WIDTH)
    # (every output absent: FEWBIT_OK behind the last refusal and before the launch)
    stops = [dict(d_gate=None, d_up=None), dict(state=P + 4)]
    singles = dict(dtype=dtypes, act=acts, bits=bits, rows=[0, BEYOND], width=[0, BEYOND], gy=pointer(1, 2, 4, 8), state=pointer(1, 2, 4), d_gate=pointer(1, 2, 4, 8, null=False),
                   d_up=pointer(1, 2, 4, 8, null=False))
    pairs = [dict(bits=3, dtype=3), dict(dtype=3, act=3), dict(act=3, rows=BEYOND), dict(d_gate=P, ld_dgate=WIDTH - 1), dict(d_up=P, ld_dup=0), {'d_gate': P, 'ld_dgate': 1, 'state': None, ALONE: True},
             dict(state=None, gy=P + 1), dict(gy=P + 2, state=P + 4), dict(dtype=BF16, gy=P + 1), dict(dtype=BF16, d_up=P + 2), dict(width=0, state=None), dict(rows=0, state=None)]
    yield Entry(lib, 'glu_backward', 'i:dtype i:act p:gy p:state z:rows z:width i:bits p:d_gate z:ld_dgate p:d_up z:ld_dup p:stream', backward, stops), singles, pairs
    yield Entry(lib, 'glu_backward_product',
                'i:dtype i:act p:gy p:state z:rows z:width i:bits p:d_gate z:ld_dgate p:d_up z:ld_dup p:product z:ld_product p:stream',
                dict(backward, product=None, ld_product=WIDTH), [dict(d_gate=None, d_up=None, product=None), dict(state=P + 4)]), \
        dict(singles, product=pointer(1, 2, 4, 8, null=False)), \
        pairs + [dict(product=P, ld_product=WIDTH - 1), dict(gy=None, d_gate=P), dict(gy=None, d_up=P + 1), dict(gy=None), dict(gy=None, state=None)]

    # ---- the normalized rows of a seed, plain and with the sum of a seed in front ----
    yield Entry(lib, 'norm_state_host', 'p:xhat_host z:rows z:width i:bits Q:seed p:out_host', dict(xhat_host=P, rows=ROWS, width=WIDTH, bits=4, seed=7, out_host=P),
                [dict(out_host=None), dict(xhat_host=None)]), \
        dict(bits=bits, width=widths, rows=[0, BEYOND], xhat_host=[None], out_host=[None]), [dict(bits=3, width=0), dict(width=8193, rows=0), dict(rows=BEYOND, xhat_host=None)]
    yield Entry(lib, 'norm_state_unpack_host', 'p:state_host z:rows z:width i:bits p:out_host', dict(state_host=P, rows=ROWS, width=WIDTH, bits=4, out_host=P),
                [dict(out_host=None), dict(state_host=None)]), \
        dict(bits=bits, width=widths, rows=[0, BEYOND], state_host=[None], out_host=[None]), [dict(bits=3, width=0), dict(rows=BEYOND, state_host=None)]
    need, space = size('norm_state_bytes', ROWS, WIDTH, 4), size('norm_workspace', ROWS, WIDTH)
    thresholds = [65536, 65537]
    for fused in (False, True):
        for kind in ('layer', 'rms'):
            centred = kind == 'layer'
            forward = dict(dtype=F32, x=P, rows=ROWS, width=WIDTH, gamma=P, eps=1e-5, bits=4, seed=7, seed_device=None, y=P, rstd=P, state=P, state_bytes=need, xhat_out=None,
                           stream=None)
            singles = dict(dtype=dtypes, width=widths, rows=[0, BEYOND], bits=bits, eps=[-1.0, float('inf'), float('nan')], seed_device=seed_word, x=pointer(1, 2, 4, 8),
                           y=pointer(1, 2, 4, 8), gamma=pointer(1, 2, 4, 8, null=False), rstd=pointer(1, 2, 4, 8), xhat_out=pointer(1, 2, 4, 8, null=False),
                           state=pointer(1, 2, 4, null=False))
            pairs = [dict(dtype=3, width=0), dict(width=8193, bits=3), dict(bits=3, eps=-1.0), dict(eps=-1.0, seed_device=P + 4), dict(seed_device=P + 4, x=None), dict(rows=0, x=None),
                     dict(rows=0, seed_device=P + 4), dict(x=None, rstd=None), dict(rstd=None, y=P + 1), dict(y=P + 2, rstd=P + 2), dict(rstd=P + 2, state=P + 4),
                     {'state': P + 4, 'state_bytes': 0, ALONE: True}, {'state_bytes': 0, ALONE: True}, dict(dtype=BF16, x=P + 1), dict(dtype=BF16, gamma=P + 2)]
            signature = 'i:dtype p:x z:rows z:width p:gamma p:beta d:eps i:bits Q:seed p:seed_device p:y p:rstd p:state z:state_bytes p:xhat_out p:stream'
            if centred:
                forward['beta'] = P
                singles['beta'] = pointer(1, 2, 4, 8, null=False)
            else:
                signature = signature.replace(' p:beta', '')
            if fused:
                signature = signature.replace('p:x ', 'p:x p:residual ').replace('p:seed_device ', 'p:seed_device u:threshold ').replace('p:y ', 'p:y p:h_out ')
                forward.update(residual=P, threshold=6554, h_out=None)
                singles.update(threshold=thresholds, residual=pointer(1, 2, 4, 8), h_out=pointer(1, 2, 4, 8, null=False))
                pairs += [dict(threshold=100, width=12), {'threshold': 0, 'width': 12, 'state_bytes': 0, ALONE: True}, dict(width=0, threshold=65536), dict(threshold=65536, bits=3),
                          dict(threshold=100, width=12, bits=3), dict(x=None, residual=None), dict(x=P + 1, residual=P + 1), dict(residual=P + 2, rstd=P + 2)]
            yield Entry(lib, ('add_' if fused else '') + kind + '_norm_forward', signature, forward, [dict(state_bytes=need - 1), dict(state=P + 4)]), singles, pairs

            backward = dict(dtype=F32, gy=P, state=P, rstd=P, gamma=P, rows=ROWS, width=WIDTH, bits=4, dgamma=P, workspace=P, workspace_bytes=space, stream=None)
            grad = 'dres' if fused else 'dx'
            backward[grad] = P
            singles = dict(dtype=dtypes, width=widths, rows=[0, BEYOND], bits=bits, gy=pointer(1, 2, 4, 8), state=pointer(1, 2, 4), rstd=pointer(1, 2, 4, 8),
                           gamma=pointer(1, 2, 4, 8, null=False), dgamma=pointer(1, 2, 4, 8, null=False), workspace=pointer(1, 2, 4, 8))
            singles[grad] = pointer(1, 2, 4, 8, null=False)
            pairs = [dict(dtype=3, width=0), dict(width=8193, bits=3), dict(bits=3, gy=None), dict(rows=0, gy=None), dict(gy=None, rstd=None), dict(rstd=None, gy=P + 1),
                     dict(gy=P + 2, rstd=P + 2), dict(rstd=P + 2, state=P + 4), dict(state=P + 4, workspace=None), dict(workspace=P + 8, workspace_bytes=0), {'workspace_bytes': 0, ALONE: True}, dict(dtype=BF16, gy=P + 1),
                     dict(dtype=BF16, gamma=P + 2)]
            signature = f'i:dtype p:gy p:state p:rstd p:gamma z:rows z:width i:bits p:{grad} p:dgamma p:dbeta p:workspace z:workspace_bytes p:stream'
            if centred:
                backward['dbeta'] = P
                singles['dbeta'] = pointer(1, 2, 4, 8, null=False)
            else:
                signature = signature.replace(' p:dbeta', '')
            if fused:
                signature = signature.replace('p:gy ', 'p:gy p:gh ').replace('i:bits ', 'i:bits Q:seed p:seed_device u:threshold ').replace('p:dres ', 'p:dres p:dbranch ')
                backward.update(gh=None, seed=7, seed_device=None, threshold=6554, dbranch=P)
                singles.update(threshold=thresholds, seed_device=seed_word, gh=pointer(1, 2, 4, 8, null=False), dbranch=pointer(1, 2, 4, 8, null=False))
                pairs += [dict(threshold=100, width=12), dict(threshold=0), {'threshold': 0, 'dbranch': None, 'workspace_bytes': 0, ALONE: True}, dict(threshold=0, seed_device=P + 4),
                          dict(seed_device=P + 4, bits=3), dict(width=0, threshold=65536), dict(dres=None, rstd=None), {'dres': None, 'dbranch': None, 'rstd': None, 'workspace_bytes': 0, ALONE: True},
                          dict(gh=P + 2, rstd=P + 2), dict(dres=P + 1, dbranch=P + 1)]
            else:
                pairs += [{'dx': None, 'rstd': None, 'workspace_bytes': 0, ALONE: True}]
            yield Entry(lib, ('add_' if fused else '') + kind + '_norm_backward', signature, backward,
                        [dict(workspace_bytes=space - 1), dict(workspace=P + 8), dict(state=P + 4)]), singles, pairs

    # ---- the mask of a seed ----
    yield Entry(lib, 'dropout_keep', 'Q:seed u:threshold Q:first z:count p:keep_host', dict(seed=7, threshold=6554, first=0, count=16, keep_host=P), [dict(keep_host=None)]), \
        dict(threshold=thresholds, count=[0]), [ {'first': 2**64 - 1, 'count': 2, 'keep_host': P, ALONE: True}, dict(threshold=65537, count=0)]
    yield Entry(lib, 'dropout', 'i:dtype p:src p:addend p:out z:n Q:first Q:seed p:seed_device u:threshold p:stream',
                dict(dtype=F32, src=P, addend=None, out=P, n=N, first=0, seed=7, seed_device=None, threshold=6554, stream=None), [dict(out=P + 1), dict(src=P + 1)]), \
        dict(dtype=dtypes, threshold=[65537], first=[1, 4, 12], seed_device=seed_word, n=[0], src=pointer(1, 2, 4, 8), addend=pointer(1, 2, 4, 8, null=False), out=pointer(1, 2, 4, 8)), \
        [dict(dtype=3, threshold=65537), dict(threshold=65537, first=1), dict(first=1, n=2**64 - 1), dict(first=8, n=2**64 - 1), dict(first=8, n=2**64 - 1, seed_device=P + 4),
         dict(seed_device=P + 4, src=None), dict(n=0, src=None), {'src': None, 'out': P + 1, ALONE: True}, dict(dtype=BF16, src=P + 1), dict(dtype=BF16, addend=P + 2, out=P + 1), dict(threshold=65536, src=None)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--library', type=Path, default=ROOT / 'fewbit_amd' / 'libfewbit_hipx.so')
    args = ap.parse_args()
    os.environ['HIP_VISIBLE_DEVICES'] = '-1'                # (nothing below may reach a device; see the docstring)
    lib = ctypes.CDLL(str(args.library))
    lib.fewbit_hipx_last_error.restype = ctypes.c_char_p
    out, ok = [], True
    for entry, singles, pairs in entries(lib):
        for bad in cases_of(entry, singles, pairs):
            ok = entry.call(lib, out, bad) and ok
    print('\n'.join(out))
    if not ok:
        print('refusal_digest: a call got as far as a launch', file=sys.stderr)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
