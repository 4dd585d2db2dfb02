"""Six seconds of tools/fuzz.py's --jpegbatch share inside the GPU suite: the batched device JPEG encoder against the single calls and the
restatement, every file byte for byte, on lists of 1 to 12 random images in random views, each with its own quality, subsampling and
restart interval, some of them cut into chunks by a small workspace budget."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

MIN_CASES = 10  # a list of twelve 96 x 96 images takes the restatement some 0.1 s on the host: a run that does fewer in 6 s did not run


def test_a_slice_of_the_jpeg_batch_fuzz():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz.py"), "--seconds", "6", "--big", "0", "--seed", "311", "--jpegbatch", "1"],
                       capture_output=True, text=True, timeout=600)
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("fuzz seed")]
    assert last, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(last[-1])
    assert r.returncode == 0 and " 0 reported" in last[-1], (r.stdout[-3000:], r.stderr[-1500:])
    assert int(last[-1].split(":")[1].split()[0]) >= MIN_CASES, last[-1]
