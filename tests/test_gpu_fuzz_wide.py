"""Twenty seconds of tools/fuzz.py's newer shares inside the GPU suite: --wide (uint16 / float32 pixels through the chain cases and the LUT
cases, against the NumPy restatement of cv2's float-weight remap) and --png (the device PNG encoder against its restatement, on remap
results and on images built to sit on the kernels' boundaries).  tests/test_gpu_fuzz.py keeps the uint8 slice."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

# cases the first run on an MI355X did in 10 s (--wide 1: 41 counted, 32 of them chain cases plus 3 over 5 % masked that do not count;
# --png 1: 755); the minimum asked for is half of that, since the oracle's and the restatements' share of the time varies with the host
MEASURED = {"--wide": 41, "--png": 755}


@pytest.mark.parametrize("seed,share", [(201, "--wide"), (202, "--png")])
def test_a_slice_of_the_wide_and_png_fuzz(seed, share):
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz.py"), "--seconds", "10", "--big", "0", "--seed", str(seed), share, "1"],
                       capture_output=True, text=True, timeout=600)
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("fuzz seed")]
    assert last, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(last[-1])
    assert r.returncode == 0 and " 0 reported" in last[-1], (r.stdout[-3000:], r.stderr[-1500:])
    assert int(last[-1].split(":")[1].split()[0]) >= MEASURED[share] // 2, last[-1]
