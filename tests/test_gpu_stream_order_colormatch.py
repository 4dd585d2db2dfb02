"""The colour-match entries on a busy stream (tests/stream_order.py has the construction): the true eyes only arrive behind a stall on
stream S, ``color_match_luts_tensor``, ``apply_luts_tensor`` and ``match_eyes_tensors`` are called on S and are back before the stall
ends, and a consumer on S sees the restatement's result of the TRUE eyes after the caller has put the decoy back into its inputs."""
import numpy as np
import pytest
import torch

import colormatch_cases as CC
import colormatch_ref as R
import stream_order as SO
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _the_construction_bites():
    SO.control(O)


def _pairs():
    true, decoy = CC.recovery_pair(11), CC.gain_pair(12)
    return list(true), list(decoy)


@pytest.mark.parametrize("mode", ["histogram", "gain"])
def test_luts_then_apply_follow_the_stream(mode):
    from vr180_convert_amd import colormatch

    true, decoy = _pairs()
    held = SO.Held(true, decoy, dsts=[((67, 131, 3), torch.uint8)])
    wluts, wreport, _ = R.luts(*true, **dict(R.DEFAULTS, mode=mode, min_pixels=16))
    want = R.apply_luts(true[1], wluts)
    assert not np.array_equal(want, R.match_eyes(*decoy, mode=mode, min_pixels=16)[0])
    s = torch.cuda.Stream()

    def call(srcs, dsts):
        luts, report = colormatch.color_match_luts_tensor(srcs[0], srcs[1], mode=mode, min_pixels=16)
        return [colormatch.apply_luts_tensor(srcs[1], luts, out=dsts[0]), luts, report]

    for _ in range(2):
        (out, luts, report), _ = held.run(s, call, launch_only=True, ms=3 * SO.STALL_MS)
        assert np.array_equal(luts, wluts) and np.array_equal(report, wreport) and np.array_equal(out, want)


def test_match_eyes_in_place_follows_the_stream():
    from vr180_convert_amd import colormatch

    true, decoy = _pairs()
    held = SO.Held(true, decoy, dsts=[((67, 131, 3), torch.uint8)])
    want = R.match_eyes(*true, min_pixels=16)[0]
    assert np.array_equal(want, true[0])  # the exact recovery
    s = torch.cuda.Stream()
    (out,), _ = held.run(s, lambda srcs, dsts: [colormatch.match_eyes_tensors(srcs[0], srcs[1], out=dsts[0], min_pixels=16)],
                         launch_only=True, ms=3 * SO.STALL_MS)
    assert np.array_equal(out, want)
    # (reuse=False: the output IS the caller's right eye; the consumer's clone is taken on S before anything else touches it)
    (out,), _ = held.run(s, lambda srcs, dsts: [colormatch.match_eyes_tensors(srcs[0], srcs[1], min_pixels=16)], launch_only=True,
                         reuse=False, ms=3 * SO.STALL_MS)
    assert np.array_equal(out, want)
