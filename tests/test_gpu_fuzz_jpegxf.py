"""Ten seconds of tools/fuzz.py's --jpegxf share under a fixed seed inside the GPU suite: the lossless JPEG composer against its
restatement -- every output's file byte for byte -- on random sets of one to four small files of one kind, joined as strips under
random codes into one or two outputs, each with its own restart interval and tables; and compositions the contract refuses, refused
the restatement's way.  A refusal by both sides alike counts as agreement; at most a third of the slice may be refusals (the
generator is tuned so that the restatement alone stays within that on this seed: DESIGN.md section 20 has the count)."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
SEED = 701


def test_a_slice_of_the_jpegxf_fuzz():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz.py"), "--seconds", "10", "--big", "0", "--seed", str(SEED), "--jpegxf", "1"],
                       capture_output=True, text=True, timeout=300)
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("fuzz seed")]
    assert last, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(last[-1])
    assert r.returncode == 0 and " 0 reported" in last[-1], (r.stdout[-3000:], r.stderr[-1500:])
    cases = int(last[-1].split(":")[1].split()[0])
    drawn, refused = (int(v) for v in last[-1].split("jpegxf cases: ")[1].replace(" drawn, ", " ").split()[:2])
    assert cases >= 10 and drawn == cases, last[-1]
    assert 3 * refused <= drawn, last[-1]
