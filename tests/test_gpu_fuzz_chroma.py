"""A few seconds of tools/fuzz.py --chroma inside the GPU suite: random chains, sizes, views, interpolations, border modes, per-unit
rotations and ChromaticAberration coefficients through remap_tensors(chromatic=) against the per-channel oracle composition, byte for
byte.  tests/test_gpu_chroma.py holds the named cases; this is a slice of the search, with a fixed seed."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_a_slice_of_the_chroma_fuzz():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz.py"), "--seconds", "6", "--seed", "7", "--chroma", "1", "--lut", "0", "--api", "0",
                        "--auto", "0", "--fused", "0"], capture_output=True, text=True, timeout=600)
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("fuzz seed")]
    assert last, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(last[-1])
    assert r.returncode == 0 and " 0 reported" in last[-1], (r.stdout[-3000:], r.stderr[-1500:])
    drawn = int(re.search(r"chroma cases: (\d+) drawn", last[-1]).group(1))
    # (the oracle's three maps per unit take most of the time, which varies with the host: only a floor)
    assert drawn >= 5, last[-1]
