"""Five seconds of tools/fuzz.py --vignette inside the GPU suite: the vignetting correction (vignette_rings_tensor,
apply_vignette_tensor) against tests/vignette_ref.py, byte for byte, on random sizes, channel counts, pixel types, pitches, offsets,
halves of a side-by-side buffer, centres inside and outside the frame, radii, coefficients, ring counts, masks and contents.
tests/test_gpu_vignette.py holds the named cases; this is a slice of the search."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_a_slice_of_the_vignette_fuzz():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz.py"), "--seconds", "5", "--big", "0", "--seed", "613", "--vignette", "1"],
                       capture_output=True, text=True, timeout=600)
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("fuzz seed")]
    assert last, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(last[-1])
    assert r.returncode == 0 and " 0 reported" in last[-1], (r.stdout[-3000:], r.stderr[-1500:])
    drawn = int(re.search(r"vignette cases: (\d+) drawn", last[-1]).group(1))
    counted = int(last[-1].split(":")[1].split()[0])
    # every case drawn is a vignette case and is counted; the restatement's share of the time varies with the host, so only a floor
    assert counted == drawn and drawn >= 10, last[-1]
