"""What the activation entry points of libfewbit_hip.so refuse, byte for byte (no GPU): tools/core_refusal_digest.py calls the four launches, the four
fewbit_hip_describe_*, fewbit_hip_tune and the two codec entry points with each bad argument in turn and with the pairs that pin which of two faults
wins, once as built and once with FEWBIT_HIP_VALIDATE=1, and its listing is compared with the committed one (profiles/core_refusal_digest.txt, recorded
from the library as it was before the unit's host code was said once).  A changed word, a changed status or a changed ORDER of two refusals fails
here.  The cases run in a child process of their own: the script lets its process see no device before the library is loaded."""
import subprocess
import sys

from helpers import ROOT


def test_core_refusals_match_the_committed_listing():
    r = subprocess.run([sys.executable, str(ROOT / 'tools' / 'core_refusal_digest.py')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = (ROOT / 'profiles' / 'core_refusal_digest.txt').read_text().splitlines()
    got = r.stdout.splitlines()
    assert len(want) > 200 and '# the same with FEWBIT_HIP_VALIDATE=1' in want      # (both parts are there: not an empty file that agrees with an empty run)
    differing = [(w, g) for w, g in zip(want, got) if w != g]
    assert not differing, differing[:5]
    assert len(got) == len(want)
