"""Ten seconds of tools/fuzz.py's --jpeg share inside the GPU suite: the device JPEG encoder against its restatement, the file byte for
byte, on remap results and random images in random views, with random quality, subsampling and restart interval."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

MIN_CASES = 50  # the restatement of a 300 x 300 image takes some 20 ms on the host: a run that does fewer in 10 s did not run


def test_a_slice_of_the_jpeg_fuzz():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz.py"), "--seconds", "10", "--big", "0", "--seed", "301", "--jpeg", "1"],
                       capture_output=True, text=True, timeout=600)
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("fuzz seed")]
    assert last, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(last[-1])
    assert r.returncode == 0 and " 0 reported" in last[-1], (r.stdout[-3000:], r.stderr[-1500:])
    assert int(last[-1].split(":")[1].split()[0]) >= MIN_CASES, last[-1]
