"""Six seconds of tools/fuzz.py's --jpegopt share inside the GPU suite: the device JPEG encoder with optimised Huffman tables against
the restatement (jpg_opt_ref.py) and the single calls, every file byte for byte, on lists of 1 to 8 random images in random views that
mix optimising and plain images, each with its own quality, subsampling and restart interval, some of them cut into chunks by a small
workspace budget; every optimised file decodes to its standard-table file's pixels and is smaller."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

MIN_CASES = 8  # a list of eight 160 x 160 images takes the restatements and Pillow some 0.3 s on the host: a run that does fewer in 6 s did not run


def test_a_slice_of_the_jpeg_optimize_fuzz():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz.py"), "--seconds", "6", "--big", "0", "--seed", "411", "--jpegopt", "1"],
                       capture_output=True, text=True, timeout=600)
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("fuzz seed")]
    assert last, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(last[-1])
    assert r.returncode == 0 and " 0 reported" in last[-1], (r.stdout[-3000:], r.stderr[-1500:])
    assert int(last[-1].split(":")[1].split()[0]) >= MIN_CASES, last[-1]
