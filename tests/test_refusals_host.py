"""What the companion library refuses, byte for byte (no GPU): tools/refusal_digest.py calls every entry point of the quant, glu, norm, fused-norm and
dropout families with each bad argument in turn and with pairs of them, and its listing is compared with the committed one
(profiles/refusal_digest.txt).  A changed word, a changed status or a changed ORDER of two refusals fails here.  The cases run in a child
process of their own: the script lets its process see no device before the library is loaded, which a process that has loaded it cannot do."""
import subprocess
import sys

from helpers import ROOT


def test_refusals_match_the_committed_listing():
    r = subprocess.run([sys.executable, str(ROOT / 'tools' / 'refusal_digest.py')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = (ROOT / 'profiles' / 'refusal_digest.txt').read_text().splitlines()
    got = r.stdout.splitlines()
    assert len(want) > 800                      # (every family is there: the listing is not an empty file that agrees with an empty run)
    differing = [(w, g) for w, g in zip(want, got) if w != g]
    assert not differing, differing[:5]
    assert len(got) == len(want)
