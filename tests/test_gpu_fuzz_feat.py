"""Ten seconds of tools/fuzz.py --feat inside the GPU suite: the feature pipeline of --automatch devfm (features.detect / features.match)
against tests/feat_ref.py on random images, views and parameters off the defaults, and the matcher on random descriptor sets.
tests/test_gpu_features_edges.py holds the named edges; this is a slice of the search."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

# counted cases of the first run on an MI355X in 10 s (205 drawn, 3 of them refused as predicted); the minimum asked for is half of that, since the NumPy restatement's share of the
# time (most of it: two detects and a brute-force match per case) varies with the host
MEASURED = 202


def test_a_slice_of_the_feat_fuzz():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz.py"), "--seconds", "10", "--big", "0", "--seed", "203", "--feat", "1"],
                       capture_output=True, text=True, timeout=600)
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("fuzz seed")]
    assert last, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(last[-1])
    assert r.returncode == 0 and " 0 reported" in last[-1], (r.stdout[-3000:], r.stderr[-1500:])
    drawn, refused = (int(v) for v in re.search(r"feat cases: (\d+) drawn, (\d+) of them refused as predicted", last[-1]).groups())
    counted = int(last[-1].split(":")[1].split()[0])
    assert counted == drawn - refused
    assert 10 * refused <= drawn, last[-1]  # (feat_ref.refusal over the drawing rule: 2.3 % of 3000 draws, tests/test_feat_host.py)
    assert counted >= MEASURED // 2 and MEASURED > 0, last[-1]
