"""The chromatic-aberration remap on a busy stream (tests/stream_order.py has the construction): the true sources only arrive behind a
stall on stream S, the entry is called on S and is back before the stall ends, and a consumer on S sees the oracle composition of the
TRUE sources after the caller has put the decoys back.  And one plan with a fix-up chain from two streams: each gets its own bytes, and
the call on the second stream is seen to wait for the first one's ray and fix-up passes (csrc/chroma.hip: flags_ev)."""
import contextlib
import time

import numpy as np
import pytest
import torch

import chainspecs as CS
import stream_order as SO
from oracle import oracle as O
from test_gpu_chroma import BLUE, RED, expect, noise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _the_construction_bites():
    O.build()
    SO.control(O)


@pytest.fixture(scope="module")
def ca():
    from vr180_convert_amd import chromatic

    return chromatic.ChromaticAberration(red=RED, blue=BLUE)


def test_the_entry_behind_a_stalled_stream_waits_for_it(ca):
    import vr180_convert_amd as V

    spec = CS.SMALL_CASES["c2_poly"][0]
    t = CS.to_product(spec)
    true, decoy = [noise(128, 128, 31), noise(128, 128, 32)], [noise(128, 128, 33), noise(128, 128, 34)]
    want = np.concatenate([expect(O, spec, im, size_output=(96, 96), radius=64.0, interp=1)[0] for im in true], axis=1)
    held = SO.Held(true, decoy, dsts=[((96, 192, 3), torch.uint8)])
    s = torch.cuda.Stream()

    def call(srcs, dsts):
        return [V.apply_lr_tensors(t, srcs[0], srcs[1], out=dsts[0], size_output=(96, 96), interpolation=1, radius=64.0, chromatic=ca)]

    with torch.cuda.stream(s):
        call(held.srcs, held.dsts)  # (the plan exists: creating one synchronises)
    s.synchronize()
    for _ in range(2):  # (the second run takes the memoised units)
        (out,), _ = held.run(s, call, launch_only=True, ms=3 * SO.STALL_MS)
        assert np.array_equal(out, want)


def test_two_streams_on_one_plan_with_a_fixup_chain(ca):
    import vr180_convert_amd as V
    from vr180_convert_amd import remapper as R

    spec = CS.SMALL_CASES["back_hemisphere"][0]
    t = CS.to_product(spec)
    imgs = [noise(256, 256, 40 + k) for k in range(4)]
    wants = [expect(O, spec, im, size_output=(256, 256), radius=128.0, interp=1)[0] for im in imgs[:2]]
    ha, hb = (SO.Held([imgs[k]], [imgs[k + 2]], [((256, 256, 3), torch.uint8)]) for k in range(2))

    def enqueue(h, late, span=None):
        if late:
            h.srcs[0].copy_(h.late[0])
        with span if span is not None else contextlib.nullcontext():
            V.remap_tensors(t, h.srcs, h.dsts, radius=128.0, interpolation=1, chromatic=ca)
        kinds = R.last_launch_kinds()
        keep = h.dsts[0].clone()
        h.srcs[0].copy_(h.decoy[0])
        SO.poison(h.dsts[0])
        return keep, kinds

    sa, sb = SO.independent_streams()
    enqueue(ha, False)  # (the plan exists)
    torch.cuda.synchronize()
    stall_ms, span = 2 * SO.STALL_MS, SO.Span()
    with torch.cuda.stream(sa):
        t_stall = time.perf_counter()
        ev = SO.stall(sa, stall_ms)
        ka, kinds_a = enqueue(ha, True)
    with torch.cuda.stream(sb):
        kb, kinds_b = enqueue(hb, True, span)
        queued = not ev.query()
    sb.synchronize()
    sa.synchronize()
    assert kinds_a == kinds_b == ["chroma+fixup"], (kinds_a, kinds_b)
    for name, keep, want in (("A", ka, wants[0]), ("B", kb, wants[1])):
        g = keep.cpu().numpy()
        assert np.array_equal(g, want), (name, int((g != want).sum()))
    assert queued
    SO.must_have_waited(span, stall_ms, t_stall, "the ray and fix-up passes on B")
