"""Ten seconds of tools/fuzz.py's --jpegprog share under a fixed seed inside the GPU suite: the device decoder of progressive JPEG
files against its restatement -- pixels byte for byte, scans, the rounds of every scan -- on random small images written progressive
by Pillow or, with a random legal scan script, by tests/jpgprog_cases.py's writer."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_a_slice_of_the_jpegprog_fuzz():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz.py"), "--seconds", "10", "--big", "0", "--seed", "501", "--jpegprog", "1"],
                       capture_output=True, text=True, timeout=300)
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("fuzz seed")]
    assert last, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(last[-1])
    assert r.returncode == 0 and " 0 reported" in last[-1], (r.stdout[-3000:], r.stderr[-1500:])
    assert int(last[-1].split(":")[1].split()[0]) >= 10, last[-1]
