#!/usr/bin/env python3
"""What the activation entry points of libfewbit_hip.so refuse, and in which words: the sibling of tools/refusal_digest.py for the four launches, the four
fewbit_hip_describe_*, fewbit_hip_tune and the two codec entry points.  Each is called through ctypes with every single bad argument in turn and with the
pairs that pin which of two faults wins, and one line per call gives the status and, where it is not FEWBIT_OK, fewbit_hip_last_error().  Two trees whose
listings agree refuse the same calls in the same order with the same bytes.

    python3 tools/core_refusal_digest.py > new.txt             # no GPU needed
    python3 tools/core_refusal_digest.py --library other/fewbit_amd/libfewbit_hip.so > old.txt
    diff old.txt new.txt

The process hides every device before the library is loaded (HIP_VISIBLE_DEVICES=-1) and ends with status 1 if the runtime still reports one.  No call can
then reach a launch or touch memory, so pointers are plain integers (P: an address that nobody owns): a launch or a describe whose arguments are all good
is refused by the device lookup ("no current HIP device"), and the codec entry points, which launch without that lookup, are never called with all
their arguments good.  Every call that is not expected to return FEWBIT_OK (n = 0, a tune key) must be refused, or the script ends with status 1.
The listing has a second part: the same cases in a child process with FEWBIT_HIP_VALIDATE=1 (the range check of every pointer, which asks the runtime).
"""
import argparse
import ctypes
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
P = 0x10000
i32, sz, vp, dbl, cp, i64 = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_double, ctypes.c_char_p, ctypes.c_longlong
F32, BF16, GELU, RELU, N = 0, 2, 2, 4, 8
BAD_DTYPES, BAD_CONTINUOUS, BAD_STEPWISE = (-1, 3), (-1, 15), (-1, 8)

# name: (signature, a call whose arguments are all good)
ENTRIES = {
    'quantize_forward': ('i:fn i:dtype p:x p:y p:state z:n p:borders i:nborders d:p0 d:p1 p:stream',
                         dict(fn=GELU, dtype=BF16, x=P, y=P, state=P, n=N, borders=P, nborders=15, p0=0.0, p1=0.0, stream=None)),
    'quantize_backward': ('i:dtype p:gy p:state p:gx z:n p:levels i:nlevels p:stream', dict(dtype=BF16, gy=P, state=P, gx=P, n=N, levels=P, nlevels=16, stream=None)),
    'stepwise1_forward': ('i:fn i:dtype p:x p:y p:state z:n d:p0 d:p1 p:stream', dict(fn=RELU, dtype=BF16, x=P, y=P, state=P, n=N, p0=0.0, p1=0.0, stream=None)),
    'stepwise1_backward': ('i:fn i:dtype p:gy p:state p:gx z:n d:p0 p:stream', dict(fn=RELU, dtype=BF16, gy=P, state=P, gx=P, n=N, p0=0.0, stream=None)),
    'describe_quantize_forward': ('i:fn i:dtype z:n i:nborders b:buf z:len', dict(fn=GELU, dtype=BF16, n=N, nborders=15, buf='buffer', len=512)),
    'describe_quantize_backward': ('i:dtype z:n i:nlevels b:buf z:len', dict(dtype=BF16, n=N, nlevels=16, buf='buffer', len=512)),
    'describe_stepwise1_forward': ('i:fn i:dtype z:n b:buf z:len', dict(fn=RELU, dtype=BF16, n=N, buf='buffer', len=512)),
    'describe_stepwise1_backward': ('i:fn i:dtype z:n b:buf z:len', dict(fn=RELU, dtype=BF16, n=N, buf='buffer', len=512)),
    'pack_codes': ('p:codes p:state z:n i:nbits p:stream', dict(codes=P, state=P, n=N, nbits=4, stream=None)),
    'unpack_codes': ('p:state p:codes z:n i:nbits p:stream', dict(state=P, codes=P, n=N, nbits=4, stream=None)),
}
KINDS = {'i': i32, 'z': sz, 'p': vp, 'd': dbl, 'b': cp}


def cases_of(name, good):
    """each single fault in turn, then the pairs that pin the order, then (where that cannot launch) the call with nothing wrong"""
    pointers = [a for a in ('x', 'y', 'gy', 'gx', 'state', 'borders', 'levels', 'codes') if a in good]
    fns = BAD_CONTINUOUS if 'quantize' in name else BAD_STEPWISE
    for dtype in BAD_DTYPES if 'dtype' in good else ():
        yield dict(dtype=dtype)
    for key, values in (('nborders', (0, 256)), ('nlevels', (1, 257)), ('nbits', (0, 9))):
        for value in values if key in good else ():
            yield {key: value}
    for fn in fns if 'fn' in good else ():
        yield dict(fn=fn)
    for p in pointers:
        yield {p: None}
    if pointers:
        yield dict({p: None for p in pointers}, n=0)               # FEWBIT_OK: nothing to do, no pointer is looked at
    if 'buf' in good:
        yield dict(buf=None)
        yield dict(len=0)
    # pairs: which of two faults wins
    table = 'nborders' if 'nborders' in good else 'nlevels' if 'nlevels' in good else None
    if table:
        yield {table: 256 if table == 'nborders' else 257, 'dtype': 3}
    if 'dtype' in good and pointers:
        yield {'dtype': 3, pointers[0]: None}
    if 'fn' in good:
        if pointers:
            yield {'fn': fns[1], pointers[0]: None}
        yield {'fn': fns[1], 'dtype': 3}
    if 'nbits' in good:
        yield {'nbits': 9, pointers[0]: None}
        yield {'nbits': 0, 'n': 0}
    if 'buf' in good:
        yield dict(buf=None, dtype=3)
    if 'codes' not in good:
        yield {}                                                  # all good: refused by the device lookup (the codec entry points have none)


def show(value):
    return 'NULL' if value is None else 'P' if value == P else repr(value)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--library', type=Path, default=ROOT / 'fewbit_amd' / 'libfewbit_hip.so')
    ap.add_argument('--validate', action='store_true', help='this process is the second part: FEWBIT_HIP_VALIDATE=1, and no third part')
    args = ap.parse_args()
    os.environ['HIP_VISIBLE_DEVICES'] = '-1'                # (nothing below may reach a device; see the docstring)
    os.environ['FEWBIT_HIP_VALIDATE'] = '1' if args.validate else '0'
    lib = ctypes.CDLL(str(args.library))
    count = i32(0)
    if ctypes.CDLL('libamdhip64.so').hipGetDeviceCount(ctypes.byref(count)) == 0 and count.value > 0:
        print('core_refusal_digest: the runtime still reports a device', file=sys.stderr)
        return 1
    lib.fewbit_hip_last_error.restype = cp
    out, ok = [], True
    buffer = ctypes.create_string_buffer(512)
    for name, (signature, good) in ENTRIES.items():
        fn = getattr(lib, 'fewbit_hip_' + name)
        params = [part.split(':') for part in signature.split()]
        fn.restype, fn.argtypes = i32, [KINDS[kind] for kind, _ in params]
        for bad in cases_of(name, good):
            values = {**good, **bad}
            status = fn(*(buffer if values[arg] == 'buffer' else values[arg] for _, arg in params))
            message = lib.fewbit_hip_last_error().decode() if status != 0 else ''
            what = ', '.join(f'{k}={show(v)}' for k, v in bad.items()) or 'nothing wrong'
            out.append(f'{name} [{what}] -> {status}' + (f' "{message}"' if status != 0 else ''))
            ok = ok and (status != 0 or bad.get('n') == 0)
    lib.fewbit_hip_tune.restype, lib.fewbit_hip_tune.argtypes = i32, [cp, i64]
    for key, value in ((None, 0), (b'no_such_key', 0), (b'chunk', -1), (b'sketch_slices', -1), (b'sketch_slices', 0), (b'sketch_waves', 5)):
        status = lib.fewbit_hip_tune(key, value)
        message = lib.fewbit_hip_last_error().decode() if status != 0 else ''
        out.append(f'tune [{"NULL" if key is None else key.decode()}, {value}] -> {status}' + (f' "{message}"' if status != 0 else ''))
    print('\n'.join(out))
    if not ok:
        print('core_refusal_digest: a call that had to be refused was not', file=sys.stderr)
        return 1
    if not args.validate:
        print('# the same with FEWBIT_HIP_VALIDATE=1', flush=True)
        return subprocess.run([sys.executable, __file__, '--library', str(args.library), '--validate']).returncode
    return 0


if __name__ == '__main__':
    sys.exit(main())
