"""tools/isa_digest.py --diff --rename: two builds compared under renamed kernel symbols (what shows that a source change which renames
kernels left their machine code alone).  The digest files are written here: no build, no GPU."""
import subprocess
import sys
from pathlib import Path

TOOL = Path(__file__).resolve().parents[1] / 'tools' / 'isa_digest.py'
RENAME = ['--rename', r'^old_(\w+)_kernel<(.*)>$=kernel<\1, \2>']


def run_diff(tmp_path, old, new, *extra):
    for name, lines in (('old.txt', old), ('new.txt', new)):
        (tmp_path / name).write_text(f'# {len(lines)} device functions\n' + ''.join(line + '\n' for line in lines))
    return subprocess.run([sys.executable, str(TOOL), '--diff', str(tmp_path / 'old.txt'), str(tmp_path / 'new.txt'), *extra], capture_output=True, text=True)


def test_renamed_identical_pair(tmp_path):
    old = ['aaaa 1111 10 old_dct_kernel<2, 16>', 'bbbb 2222 20 other<1>']
    new = ['aaaa 1111 10 kernel<dct, 2, 16>', 'bbbb 2222 20 other<1>']
    plain = run_diff(tmp_path, old, new)
    assert plain.returncode == 0 and 'removed 1, added 1, identical 1,' in plain.stdout
    mapped = run_diff(tmp_path, old, new, *RENAME)
    assert mapped.returncode == 0, mapped.stderr
    assert mapped.stdout.splitlines() == ['2 device functions before, 2 after; removed 0, added 0, identical 2, same instructions in another order 0, different instructions 0']


def test_renamed_changed_pair(tmp_path):
    old = ['aaaa 1111 10 old_dct_kernel<2, 16>', 'cccc 3333 12 old_dft_kernel<2, 16>']
    new = ['aaab 1112 11 kernel<dct, 2, 16>', 'cccd 3333 12 kernel<dft, 2, 16>']
    mapped = run_diff(tmp_path, old, new, *RENAME)
    assert mapped.returncode == 1                  # other instructions in one kernel
    lines = mapped.stdout.splitlines()
    assert lines[0].endswith('removed 0, added 0, identical 0, same instructions in another order 1, different instructions 1')
    assert any(line.startswith('CHANGED') and line.endswith('kernel<dct, 2, 16>') for line in lines)
    assert any(line.startswith('reordered') and line.endswith('kernel<dft, 2, 16>') for line in lines)


def test_collision_is_an_error(tmp_path):
    old = ['aaaa 1111 10 old_dct_kernel<2, 16>', 'cccc 3333 12 kernel<dct, 2, 16>']
    new = ['aaaa 1111 10 kernel<dct, 2, 16>']
    mapped = run_diff(tmp_path, old, new, *RENAME)
    assert mapped.returncode == 2
    assert 'old_dct_kernel<2, 16>' in mapped.stderr and 'are both named kernel<dct, 2, 16>' in mapped.stderr
    assert mapped.stdout == ''
