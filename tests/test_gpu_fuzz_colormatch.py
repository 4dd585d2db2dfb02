"""Five seconds of tools/fuzz.py --colormatch inside the GPU suite: the colour match of two eyes (color_match_luts_tensor,
apply_luts_tensor) against tests/colormatch_ref.py, byte for byte, on random sizes, channel counts, pitches, offsets, halves of a
side-by-side buffer, modes, references, parameters and contents.  tests/test_gpu_colormatch.py holds the named cases; this is a slice of
the search."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_a_slice_of_the_colormatch_fuzz():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz.py"), "--seconds", "5", "--big", "0", "--seed", "512", "--colormatch", "1"],
                       capture_output=True, text=True, timeout=600)
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("fuzz seed")]
    assert last, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(last[-1])
    assert r.returncode == 0 and " 0 reported" in last[-1], (r.stdout[-3000:], r.stderr[-1500:])
    drawn = int(re.search(r"colormatch cases: (\d+) drawn", last[-1]).group(1))
    counted = int(last[-1].split(":")[1].split()[0])
    # every case drawn is a colormatch case and is counted; the restatement's share of the time varies with the host, so only a floor
    assert counted == drawn and drawn >= 10, last[-1]
