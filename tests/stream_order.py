"""The stall: a busy stream for the tests of stream order (tests/test_gpu_stream_order.py, tests/test_gpu_stream_order_codecs.py).

Every other GPU test hands an entry point inputs that are resident and looks at the result behind a synchronisation, so work on the
wrong stream, a read in front of the stream's turn or a missing event wait all pass.  Here the stream is made busy BEFORE the call:

    src holds a DECOY                       # another valid input of the same shape: nothing errors on it
    stall(S); src.copy_(true)               # the true input only arrives on S, behind the delay
    f(..., stream=S)                        # everything f enqueues waits behind both
    assert not stall_event.query()          # launch-only entries: the call is back and its work has not begun
    keep = out.clone()                      # a consumer on S, no host synchronisation in between
    src.copy_(decoy); out.fill_(0xA5)       # the caller reuses its buffers at once
    S.synchronize(); keep == expected(true) # expected: the oracle / the restatements, never an unstalled run of the product

``stall(stream, ms)`` is ``torch.cuda._sleep`` with a cycle count calibrated once per process by a pair of timing events (a chain of
4096 x 4096 ``torch.mm`` launches, timed the same way, where the sleep returns at once; neither: the module FAILS).  The delay always
ends by itself -- no kernel waits for anything the host sets --, is never longer than 250 ms, and a stream carries one at a time.

Length: STALL_MS = 20 per call queued behind the stall.  profiles/stream_order/README.md has the calibration on an MI355X, the host time
of every launch-only call at the tests' shapes (the slowest 0.165 ms: ten times that is below the issue's floor of 20 ms) and how both
were measured (tools/stream_order_times.py).  The sequences that queue several calls behind ONE stall ask for 20 ms per queued call.

``Span`` and ``must_have_waited`` hold a call on a second stream B to the observable effect of an event wait on the stalled stream A:
timing events on B around the call must be apart by what was left of A's stall.  B is idle, so without the wait the call runs at
once and the span is the kernels' own time, a fraction of a millisecond.

``independent(a, b)``: two torch streams can share a hardware queue, and then a stall on one delays the other -- a two-stream test would
pass without having run anything side by side.  ``independent_streams()`` tries up to four fresh partners and fails where none runs
beside the stalled stream.

``control()`` shows that the construction bites, with no change to the library: ``v1c_remap_lut`` with ``stream = NULL`` while its source
only becomes right behind a stall on a side stream (torch's side streams do not block against the null stream).  The result must be
the DECOY's; the true one means a late input discriminates nothing here, and both modules fail."""
from __future__ import annotations

import math
import time

import analytic_ref as A
import chainspecs as CS
import numpy as np
import pytest
import torch

STALL_MS = 20.0        # one call queued behind the stall (see above)
MAX_STALL_MS = 250.0   # no single delay is longer
CAL_CYCLES = 4_000_000
POISON = 0xA5

_CAL: dict = {}
_PENDING: dict = {}    # stream handle -> the event behind its last stall
_CONTROL: dict = {}


def _timed(stream, fn) -> float:
    """milliseconds between two events around fn() on ``stream``"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        fn()
        e1.record()
    e1.synchronize()
    return float(e0.elapsed_time(e1))


def calibration() -> dict:
    """{'kind': 'sleep', 'cycles_per_ms': ...} or {'kind': 'mm', 'ms_per_launch': ...}, measured once per process"""
    if _CAL:
        return _CAL
    s = torch.cuda.Stream()
    _timed(s, lambda: torch.cuda._sleep(1000))  # (the kernel is resident)
    ms = sorted(_timed(s, lambda: torch.cuda._sleep(CAL_CYCLES)) for _ in range(3))[1]
    if ms >= 0.5:
        _CAL.update(kind="sleep", cycles_per_ms=CAL_CYCLES / ms, measured_ms=ms)
        return _CAL
    a = torch.randn((4096, 4096), device="cuda")
    c = torch.empty_like(a)
    _timed(s, lambda: torch.mm(a, a, out=c))
    per = sorted(_timed(s, lambda: [torch.mm(a, a, out=c) for _ in range(4)]) for _ in range(3))[1] / 4
    if per >= 0.05:
        _CAL.update(kind="mm", ms_per_launch=per, a=a, c=c, sleep_ms=ms)
        return _CAL
    pytest.fail(f"no device-side delay: torch.cuda._sleep({CAL_CYCLES}) took {ms:.3f} ms and a 4096^3 torch.mm {per:.3f} ms")


def stall(stream, ms: float | None = None):
    """a delay of ``ms`` on ``stream`` that ends by itself; the event recorded behind it"""
    ms = STALL_MS if ms is None else float(ms)
    assert 0 < ms <= MAX_STALL_MS, ms
    cal = calibration()
    prev = _PENDING.get(stream.cuda_stream)
    assert prev is None or prev.query(), "a stream carries one delay at a time"
    with torch.cuda.stream(stream):
        if cal["kind"] == "sleep":
            torch.cuda._sleep(int(ms * cal["cycles_per_ms"]))
        else:
            for _ in range(math.ceil(ms / cal["ms_per_launch"])):
                torch.mm(cal["a"], cal["a"], out=cal["c"])
        ev = torch.cuda.Event()
        ev.record()
    _PENDING[stream.cuda_stream] = ev
    return ev


def independent(a, b) -> bool:
    """while ``a`` is stalled, an event recorded on ``b`` completes before a's stall does"""
    ev = stall(a)
    eb = torch.cuda.Event()
    eb.record(b)
    eb.synchronize()
    beside = not ev.query()
    a.synchronize()
    return beside


def independent_streams():
    """(a, b): two streams of which b has been seen to run while a was stalled"""
    a = torch.cuda.Stream()
    tried = []
    for _ in range(4):
        b = torch.cuda.Stream()
        tried.append(b)
        if independent(a, b):
            return a, b
    pytest.fail("four fresh torch streams each waited for the stalled one: they share its hardware queue, and a two-stream test "
                "would not run anything side by side")


class Span:
    """timing events on the current stream around the calls made inside the ``with`` block, and the host time of the first"""

    def __init__(self):
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.t0 = None

    def __enter__(self):
        self.t0 = time.perf_counter()
        self.e0.record()
        return self

    def __exit__(self, *exc):
        self.e1.record()

    def ms(self) -> float:
        self.e1.synchronize()
        return float(self.e0.elapsed_time(self.e1))


def must_have_waited(span: Span, stall_ms: float, t_stall: float, what: str) -> None:
    """The calls inside ``span``, made on an idle stream, waited for a stream whose stall of ``stall_ms`` was enqueued at host time
    ``t_stall`` (``time.perf_counter()`` taken just before ``stall()``).  The stall begins no earlier than ``t_stall`` and the span's first
    event is recorded at ``span.t0``, so at least ``left = stall_ms - (span.t0 - t_stall)`` ms of it lay ahead.  The span must cover
    ``left`` less a slack of a tenth of the stall plus 1 ms: the calibration reproduces 20 / 100 / 250 ms within 0.5 % and an event on
    an idle stream completes within tens of microseconds of its record, so the slack is several times what either can take away.
    Without a wait the span is the call's own kernels, well under a millisecond.  A host so slow that less than half the stall is left
    fails the test as inconclusive."""
    left = stall_ms - (span.t0 - t_stall) * 1e3
    assert left >= stall_ms / 2, f"{what}: only {left:.1f} ms of the {stall_ms} ms stall were left when the call was made: inconclusive"
    got = span.ms()
    print(f"{what}: the span on the second stream is {got:.2f} ms, {left:.2f} ms of the stall were left")
    assert got >= left - (0.1 * stall_ms + 1.0), (f"{what}: the call on the second stream took {got:.2f} ms while {left:.2f} ms of the first "
                                                 "stream's stall were left: it did not wait for the first stream's launch")


# ---- shapes shared by the two-stream tests and tools/stream_order_times.py -------------------------------------------------------------
ROT_BASE = [("equirect_enc", True), ("rot_quat", (1.0, 0.0, 0.0, 0.0)), CS.EQUI]
AUTO_SPEC = [("equirect_enc", True), ("poly", [0, 1, -0.05]), CS.EQUI]


def rot_units(n, seed, first=0):
    """n noise sources of 160 x 160 with a calibration rotation each (the geometry of test_more_units_than_a_ring_slot_holds)"""
    return [A.noise(np.uint8, 160, 160, 3, seed + k) for k in range(n)], [CS.c5_spec((first + f) // 2, (first + f) % 2) for f in range(n)]


def discs(seed, r0, r1, size=360):
    """two image circles on black of the radii given, the second off centre (tests/test_gpu_analytic.py: what get_radius can find)"""
    yy, xx = np.mgrid[0:size, 0:size]
    out = []
    for k, (r, cx) in enumerate(((r0, size / 2), (r1, size / 2 - 4))):
        img = np.maximum(A.noise(np.uint8, size, size, 3, seed + k), 40)
        img[(xx - cx) ** 2 + (yy - size / 2) ** 2 > r * r] = 0
        out.append(img)
    return out


def poison(t: torch.Tensor) -> None:
    """0xA5 in every byte, whatever the type"""
    (t.view(torch.uint8) if t.is_contiguous() else t).fill_(POISON)


def up(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


class Held:
    """The buffers of one entry held to the pattern: ``srcs`` hold the decoys, the true inputs wait on the device beside them, ``dsts``
    (optional, ``(shape, dtype)`` each) are the caller's outputs.  The buffers are the same in every run, so a second run takes the
    product's memoised path."""

    def __init__(self, true, decoy, dsts=()):
        assert len(true) == len(decoy) and all(t.shape == d.shape and t.dtype == d.dtype and not np.array_equal(t, d) for t, d in zip(true, decoy))
        self.late = [up(a) for a in true]
        self.decoy = [up(a) for a in decoy]
        self.srcs = [d.clone() for d in self.decoy]
        self.dsts = [torch.empty(shape, dtype=dtype, device="cuda") for shape, dtype in dsts]
        torch.cuda.synchronize()

    def run(self, stream, call, *, launch_only: bool, reuse: bool = True, ms: float | None = None):
        """``call(srcs, dsts)`` -> the output tensors, made with ``stream`` current and busy.  Returns (outputs as numpy arrays, whether
        the call came back with the stall still in force); ``launch_only`` asserts the latter."""
        with torch.cuda.stream(stream):
            for d in self.dsts:
                poison(d)
            ev = stall(stream, ms)
            for s, t in zip(self.srcs, self.late):
                s.copy_(t)
            outs = list(call(self.srcs, self.dsts))
            queued = not ev.query()
            keep = [o.clone() for o in outs]
            if reuse:
                for s, d in zip(self.srcs, self.decoy):
                    s.copy_(d)
                for o in outs:
                    poison(o)
        stream.synchronize()
        got = [k.cpu().numpy() for k in keep]
        if launch_only:
            assert queued, "the call came back only after the stall had run out: it waited for the stream"
        return got, queued


def control(oracle_mod) -> None:
    """see the module's docstring; runs once per process, both modules ask for it"""
    if _CONTROL:
        assert _CONTROL["ok"], _CONTROL["why"]
        return
    from vr180_convert_amd import _native
    from vr180_convert_amd.remapper import border_scalar

    rng = np.random.default_rng(20251)
    true, decoy = (rng.integers(0, 256, (40, 60, 3), dtype=np.uint8) for _ in range(2))
    xm = rng.uniform(0, 59, (48, 64)).astype(np.float32)
    ym = rng.uniform(0, 39, (48, 64)).astype(np.float32)
    want_true, want_decoy = (oracle_mod.remap(a, xm, ym, 1, 0, 0) for a in (true, decoy))
    assert not np.array_equal(want_true, want_decoy)
    src, late, x_d, y_d = up(decoy), up(true), up(xm), up(ym)
    out = torch.zeros((48, 64, 3), dtype=torch.uint8, device="cuda")
    bv = border_scalar(0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ev = stall(side)
    with torch.cuda.stream(side):
        src.copy_(late)
    rc = _native.lib().v1c_remap_lut(0, None, src.data_ptr(), 40, 60, 180, 3, out.data_ptr(), 48, 64, 192, x_d.data_ptr(), y_d.data_ptr(), 256,
                                     1, 0, bv.ctypes.data)
    _native.check(rc, "v1c_remap_lut")
    got = out.cpu().numpy()  # (torch's default stream is the null stream: behind the launch)
    side.synchronize()
    assert ev.query()
    if np.array_equal(got, want_true):
        _CONTROL.update(ok=False, why="a launch on the null stream saw the input that only arrives behind the stall of a side stream: the "
                                      "construction discriminates nothing here")
    elif not np.array_equal(got, want_decoy):
        _CONTROL.update(ok=False, why="the control's output is neither the decoy's nor the true input's")
    else:
        _CONTROL.update(ok=True, why="")
    assert _CONTROL["ok"], _CONTROL["why"]
