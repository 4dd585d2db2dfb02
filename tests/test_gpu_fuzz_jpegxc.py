"""Ten seconds of tools/fuzz.py's --jpegxc share under a fixed seed inside the GPU suite: the lossless JPEG transcoder against its
restatement -- every output's file byte for byte -- on random small images of random sampling, quality and restart interval cut into
random lists of regions (crops, splits, swaps, shuffled strips), each output with its own restart interval and tables; and lists the
contract refuses, refused the restatement's way."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_a_slice_of_the_jpegxc_fuzz():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz.py"), "--seconds", "10", "--big", "0", "--seed", "601", "--jpegxc", "1"],
                       capture_output=True, text=True, timeout=300)
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("fuzz seed")]
    assert last, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(last[-1])
    assert r.returncode == 0 and " 0 reported" in last[-1], (r.stdout[-3000:], r.stderr[-1500:])
    assert int(last[-1].split(":")[1].split()[0]) >= 10, last[-1]
