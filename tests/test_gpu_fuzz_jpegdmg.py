"""Forty cases of tools/fuzz.py's --jpegdmg share under a fixed seed inside the GPU suite: the device JPEG decoders on a random small
image with a random encoder setting, ONE random damage inside a scan (tests/jpgdmg_cases.py's kinds) and a random subsequence size,
held to the restatement's verdict -- the code, the smallest bad bit and its scan, the rounds, and the pixels of damage that is still
a legal stream.  tests/test_jpegdmg_host.py runs the same forty cases through the host builds first."""
import subprocess
import sys
from pathlib import Path

import pytest

import jpgdmg_cases as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_a_slice_of_the_jpegdmg_fuzz():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz.py"), "--seconds", "120", "--cases", str(M.FUZZ_CASES), "--big", "0", "--seed",
                        str(M.FUZZ_SEED), "--jpegdmg", "1"], capture_output=True, text=True, timeout=600)
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("fuzz seed")]
    assert last, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(last[-1])
    assert r.returncode == 0 and " 0 reported" in last[-1], (r.stdout[-3000:], r.stderr[-1500:])
    assert int(last[-1].split(":")[1].split()[0]) == M.FUZZ_CASES, last[-1]
    share = last[-1].split("jpegdmg cases: ")[1]
    assert int(share.split(" drawn")[0]) == M.FUZZ_CASES, last[-1]
    assert int(share.split(" refused by the last pass")[0].split(", ")[-1]) >= 10 and int(share.split(" decoded")[0].split(", ")[-1]) >= 5, last[-1]
