"""Forty cases of tools/fuzz.py's --jpegdec share under a fixed seed inside the GPU suite: the device JPEG decoder against its
restatement, the pixels byte for byte, on random small images with random sampling, quality, restart setting, optimised tables and
subsequence size."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

CASES = 40


def test_a_slice_of_the_jpegdec_fuzz():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz.py"), "--seconds", "120", "--cases", str(CASES), "--big", "0", "--seed", "401",
                        "--jpegdec", "1"], capture_output=True, text=True, timeout=600)
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("fuzz seed")]
    assert last, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(last[-1])
    assert r.returncode == 0 and " 0 reported" in last[-1], (r.stdout[-3000:], r.stderr[-1500:])
    assert int(last[-1].split(":")[1].split()[0]) == CASES, last[-1]
