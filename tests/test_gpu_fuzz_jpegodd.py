"""Ten seconds of tools/fuzz.py's --jpegodd share under a fixed seed inside the GPU suite: the device JPEG decoders on legal files of
unusual structure (drawn Huffman code shapes and table slots, quantisation slots and widths, component ids, segment orders, fill bytes,
DRI oddities) and on small files with ONE damage in a marker segment, held to the restatement: the parse's class, then the code, the
bad bit, the rounds and the pixels.  tests/test_jpegdmg_host.py runs the same cases through the host builds first."""
import subprocess
import sys
from pathlib import Path

import pytest

import jpgodd_cases as O

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_a_slice_of_the_jpegodd_fuzz():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz.py"), "--seconds", "10", "--cases", str(O.FUZZ_CASES), "--big", "0", "--seed",
                        str(O.FUZZ_SEED), "--jpegodd", "1"], capture_output=True, text=True, timeout=300)
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("fuzz seed")]
    assert last, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(last[-1])
    assert r.returncode == 0 and " 0 reported" in last[-1], (r.stdout[-3000:], r.stderr[-1500:])
    assert int(last[-1].split(":")[1].split()[0]) >= 10, last[-1]
