"""The vignetting entries on a busy stream (tests/stream_order.py has the construction): the true image only arrives behind a stall on
stream S, ``apply_vignette_tensor`` and ``vignette_rings_tensor`` are called on S and are back before the stall ends, and a consumer
on S sees the restatement's result of the TRUE image after the caller has put the decoy back into its input."""
import numpy as np
import pytest
import torch

import stream_order as SO
import vignette_cases as VC
import vignette_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu
CENTER, RADIUS = (40, 19), 44.0


@pytest.fixture(scope="module", autouse=True)
def _the_construction_bites():
    SO.control(O)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_apply_and_rings_follow_the_stream(dtype):
    from vr180_convert_amd import vignette as V

    true, decoy = VC.noise(37, 83, 3, dtype, 81), VC.noise(37, 83, 3, dtype, 82)
    v = VC.carve(np.zeros((1, 1, 3), dtype), coefs=VC.STRONG).vignette()
    g = V.geometry(37, 83, CENTER, RADIUS)
    lo, hi = V.default_mask(dtype)
    want = R.apply(true, V.gain_tables(v), g.cx, g.cy, g.scale, g.shift)
    wrec = R.rings(true, g.cx, g.cy, V.ring_r2(RADIUS), 64, lo, hi)
    assert not np.array_equal(want, R.apply(decoy, V.gain_tables(v), g.cx, g.cy, g.scale, g.shift))
    assert not np.array_equal(wrec, R.rings(decoy, g.cx, g.cy, V.ring_r2(RADIUS), 64, lo, hi))
    tables = V.tables_tensor(v, "cuda")  # (resident before the stream is made busy: an upload would wait for the stall)
    held = SO.Held([true], [decoy], dsts=[((37, 83, 3), torch.uint8 if dtype == np.uint8 else torch.uint16)])
    s = torch.cuda.Stream()

    def call(srcs, dsts):
        rec = V.vignette_rings_tensor(srcs[0], center=CENTER, radius=RADIUS, rings=64)
        return [V.apply_vignette_tensor(srcs[0], None, center=CENTER, radius=RADIUS, out=dsts[0], tables=tables), rec]

    for _ in range(2):
        (out, rec), _ = held.run(s, call, launch_only=True, ms=2 * SO.STALL_MS)
        assert np.array_equal(out, want) and np.array_equal(rec, wrec)


def test_in_place_follows_the_stream():
    from vr180_convert_amd import vignette as V

    true, decoy = VC.noise(37, 83, 4, np.uint8, 83), VC.noise(37, 83, 4, np.uint8, 84)
    v = VC.carve(np.zeros((1, 1, 3), np.uint8), coefs=VC.ENCODED).vignette()
    g = V.geometry(37, 83, CENTER, RADIUS)
    want = R.apply(true, V.gain_tables(v), g.cx, g.cy, g.scale, g.shift)
    tables = V.tables_tensor(v, "cuda")
    held = SO.Held([true], [decoy])
    s = torch.cuda.Stream()
    # (reuse=False: the output IS the caller's image; the consumer's clone is taken on S before anything else touches it)
    (out,), _ = held.run(s, lambda srcs, dsts: [V.apply_vignette_tensor(srcs[0], None, center=CENTER, radius=RADIUS, out=srcs[0], tables=tables)],
                         launch_only=True, reuse=False)
    assert np.array_equal(out, want)
