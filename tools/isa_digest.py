#!/usr/bin/env python3
"""Per-kernel digests of the gfx950 machine code in the built objects (fewbit_amd/csrc/build/gfx950/*.o): the device code object
is taken out of each object's .hip_fatbin, disassembled with llvm-objdump, and every kernel's instruction text is hashed
(addresses and encodings dropped), once in program order and once sorted (the instruction multiset).  Two builds whose digests
agree run the same instructions: how a source clean-up is shown to change no bit of output.

    python3 tools/isa_digest.py [build dir] > digests.txt         # one line per kernel: <sha256[:16] in order> <sha256[:16] sorted> <instructions> <symbol>
    python3 tools/isa_digest.py --diff old.txt new.txt            # what differs (kernels added / removed / changed)
    python3 tools/isa_digest.py --diff old.txt new.txt --rename 'regex=replacement' [--rename ...]
                                                                  # the same after a source change that renames kernels: every symbol of BOTH files goes
                                                                  # through re.sub(regex, replacement) of each --rename in turn (kernels are then "removed"
                                                                  # and "added" only if the map misses them); two symbols of one file under one name: exit 2
    python3 tools/isa_digest.py --where old_build new_build       # WHERE each changed streaming kernel differs: only behind its tile loop, or in it

--where is for a change that is meant to touch the element-wise tail of the streaming activation kernels (fewbit_kernels.hip) and nothing else.  The
tile loop of such a kernel is what lies between its first and its last 16-byte memory instruction (global_load / global_store_dwordx4: the tails use
byte, short and dword accesses only).  Every kernel whose instruction text differs gets one line:
    tail only    the two texts are identical from the first instruction up to and beyond the last 16-byte access
    renumbered   they differ earlier, but the tile loop is the same instruction sequence once registers are renamed in order of first use
    LOOP CHANGED neither
with the instruction counts, the registers and the scratch bytes of the kernel's metadata before and after.
"""
import hashlib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path('/opt/rocm/lib/llvm/bin')
ROOT = Path(__file__).resolve().parents[1]


def code_object(obj: Path, tmp: str) -> Path:
    """the gfx950 code object inside a host object's .hip_fatbin"""
    fat, co = Path(tmp) / (obj.stem + '.fatbin'), Path(tmp) / (obj.stem + '.co')
    subprocess.run([LLVM / 'llvm-objcopy', '-O', 'binary', '--only-section=.hip_fatbin', obj, fat], check=True)
    subprocess.run([LLVM / 'clang-offload-bundler', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', f'--input={fat}', f'--output={co}', '--unbundle'], check=True)
    return co


def digests(build: Path):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(build.glob('*.o')):
            co = code_object(obj, tmp)
            text = subprocess.run([LLVM / 'llvm-objdump', '-d', co], check=True, capture_output=True, text=True).stdout
            name, body = None, []

            def flush():
                if name is not None:
                    out[name] = (hashlib.sha256('\n'.join(body).encode()).hexdigest()[:16], hashlib.sha256('\n'.join(sorted(body)).encode()).hexdigest()[:16], len(body))
            for line in text.splitlines():
                m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
                if m:
                    flush()
                    name, body = m.group(1), []
                elif name is not None and line.startswith('\t'):
                    body.append(re.sub(r'\s*//.*$', '', line).strip())
            flush()
    return out


def listings(build: Path, pattern: str = 'fewbit_kernels*.o'):
    """{kernel: (instruction text, 'vgpr / sgpr / scratch bytes' of its metadata)} of the objects of a build that match `pattern`"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(build.glob(pattern)):
            co = code_object(obj, tmp)
            notes = subprocess.run([LLVM / 'llvm-readelf', '--notes', co], check=True, capture_output=True, text=True).stdout
            use = {m.group(1): f'{m.group(4)} v / {m.group(3)} s / {m.group(2)} B'
                   for m in re.finditer(r'\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)\n\s+\.sgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)', notes)}
            text = subprocess.run([LLVM / 'llvm-objdump', '-d', co], check=True, capture_output=True, text=True).stdout
            name = None
            for line in text.splitlines():
                m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
                if m:
                    name = m.group(1)
                    out[name] = ([], use.get(name, '?'))
                elif name is not None and line.startswith('\t'):
                    out[name][0].append(re.sub(r'\s*//.*$', '', line).strip())
    return out


def tile_loop(body):
    """first .. last 16-byte memory instruction, registers renamed in order of first use, branch distances dropped"""
    wide = [i for i, l in enumerate(body) if 'dwordx4' in l and l.startswith('global_')]
    names = {}

    def reg(kind, i):
        return names.setdefault((kind, i), f'{kind}#{len(names)}')
    out = []
    for l in body[wide[0]:wide[-1] + 1] if wide else []:
        if l.startswith(('s_branch', 's_cbranch')):
            l = l.split()[0]
        l = re.sub(r'\b([vsa])\[(\d+):(\d+)\]', lambda g: '[' + ','.join(reg(g.group(1), i) for i in range(int(g.group(2)), int(g.group(3)) + 1)) + ']', l)
        out.append(re.sub(r'\b([vsa])(\d+)\b', lambda g: reg(g.group(1), int(g.group(2))), l))
    return out


def where(old: Path, new: Path) -> int:
    a, b = listings(old), listings(new)
    rows = []
    for k in sorted(a.keys() & b.keys()):
        (ta, ua), (tb, ub) = a[k], b[k]
        if ta == tb:
            continue
        same = next((i for i, (x, y) in enumerate(zip(ta, tb)) if x != y), min(len(ta), len(tb)))
        last = max((i for i, l in enumerate(ta) if 'dwordx4' in l and l.startswith('global_')), default=-1)
        verdict = 'tail only   ' if same > last else 'renumbered  ' if tile_loop(ta) == tile_loop(tb) else 'LOOP CHANGED'
        rows.append((verdict, f'{verdict} {len(ta):5d} -> {len(tb):5d} instructions, identical up to {same:4d}, last 16-byte access at {last:4d}; {ua} -> {ub}  {k}'))
    count = {v: sum(r[0] == v for r in rows) for v in ('tail only   ', 'renumbered  ', 'LOOP CHANGED')}
    print(f'{len(a)} kernels before, {len(b)} after, {len(rows)} with another instruction text: ' + ', '.join(f'{n} {v.strip()}' for v, n in count.items()))
    for _, line in rows:
        print(line)
    return 1 if count['LOOP CHANGED'] else 0


def read_digests(path, renames):
    """{symbol: [digest in order, digest sorted, instructions]} of a digest file, each symbol after every `regex=replacement` of `renames`
    in turn (re.sub); two symbols of the file that end under one name are an error: one would hide the other from the comparison"""
    out, source = {}, {}
    for line in open(path):
        if not line.strip() or line.startswith('#'):
            continue
        *fields, symbol = line.split(' ', 3)
        symbol = name = symbol.strip()
        for pattern, replacement in renames:
            name = re.sub(pattern, replacement, name)
        if name in out:
            raise ValueError(f'{path}: {source[name]} and {symbol} are both named {name}')
        out[name], source[name] = fields, symbol
    return out


def diff(old, new, renames=()) -> int:
    try:
        a, b = read_digests(old, renames), read_digests(new, renames)
    except ValueError as e:
        print(f'error: {e}', file=sys.stderr)
        return 2
    changed = [k for k in a if k in b and a[k][0] != b[k][0]]
    reordered = [k for k in changed if a[k][1] == b[k][1]]
    print(f'{len(a)} device functions before, {len(b)} after; removed {len(a.keys() - b.keys())}, added {len(b.keys() - a.keys())}, identical {len([k for k in a if k in b]) - len(changed)}, '
          f'same instructions in another order {len(reordered)}, different instructions {len(changed) - len(reordered)}')
    for k in sorted(a.keys() - b.keys()):
        print('removed', k)
    for k in sorted(b.keys() - a.keys()):
        print('added  ', k)
    for k in changed:
        print('reordered' if k in reordered else 'CHANGED  ', a[k], '->', b[k], k)
    return 1 if len(changed) > len(reordered) else 0


def main():
    if len(sys.argv) > 3 and sys.argv[1] == '--where':
        return where(Path(sys.argv[2]), Path(sys.argv[3]))
    if len(sys.argv) > 1 and sys.argv[1] == '--diff':
        args, renames = sys.argv[2:], []
        while '--rename' in args:
            at = args.index('--rename')
            renames.append(args[at + 1].split('=', 1))
            del args[at:at + 2]
        return diff(args[0], args[1], renames)
    build = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / 'fewbit_amd' / 'csrc' / 'build' / 'gfx950'
    d = digests(build)
    print(f'# {len(d)} device functions in {build}')
    for k, (h, hs, n) in sorted(d.items()):
        print(h, hs, n, k)
    return 0


if __name__ == '__main__':
    sys.exit(main())
