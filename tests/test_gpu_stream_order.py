"""The remap family held to stream order on a busy stream (tests/stream_order.py states the construction): every entry that takes a
stream is called while that stream is stalled, its input only becomes right behind the stall, a consumer reads the output on the same
stream and the caller overwrites its buffers at once -- and the bytes are the oracle's for the true input.  One case per kernel family
at the smallest geometry the suite reaches it with (asserted with ``last_launch_kinds``), each once cold (the plan is created while the
stream is busy) and once warm (the memoised path, where the launch-only calls must come back with the stall still in force).

Then the sequences nothing else reaches: more launches through the plan's unit ring than it has slots behind ONE stall; and, from one
thread on two streams that were seen to run side by side, the three pieces of plan state that only an event wait orders across
streams (csrc/plan.hip): the ring slots, the tile-flag words between the ray pass and the fix-up pass, and the plan-resident context
that ``v1c_plan_run_auto*`` rewrites.  The stalled stream A is enqueued first and waits for nothing of B's; B waits, through the
plan's event, for A's delay, which ends by itself.  Since all of A's work, its writes of the shared state included, sits behind its
stall, B would not corrupt anything without the wait: these cases assert the wait's observable effect, that the call on B is seen to
take as long as what was left of A's stall, beside the bytes of both streams."""
import contextlib
import ctypes as C
import time

import numpy as np
import pytest
import torch

import analytic_ref as A
import chainspecs as CS
import stream_order as SO
from stream_order import AUTO_SPEC, ROT_BASE, discs, rot_units
import test_analytic_remap as T
import wide_ref as W
from test_gpu_analytic import C0, EQUI, WANTED
from test_gpu_mirror_record import PAIR_CASES, frames
from test_gpu_parity import LEAN_BATCH
from test_oracle_golden import assert_maps_match

pytestmark = pytest.mark.gpu

_REACHED: set = set()   # kernel families served behind a stall (the names of test_gpu_analytic.WANTED)
COLD_CALLS_THAT_CREATE_A_PLAN = ["batch", "cn 1", "cn 4", "kxk-auto", "mirror pair", "mirror single", "rot_pair", "tile interp 2", "tile interp 4",
                                 "wide float32", "wide uint16"]
_LATE_RETURNS: list = []  # launch-only entries whose COLD call came back after the stall (plan creation synchronises the device)


@pytest.fixture(scope="module")
def V():
    import vr180_convert_amd as V
    from vr180_convert_amd import _native

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    _native.lib()
    return V


@pytest.fixture(scope="module")
def R(V):
    from vr180_convert_amd import remapper

    return remapper


@pytest.fixture(scope="module")
def lib(V):
    from vr180_convert_amd import _native

    return _native.lib()


@pytest.fixture(scope="module", autouse=True)
def _the_construction_bites(V, oracle_mod):
    SO.control(oracle_mod)


@pytest.fixture(scope="module")
def S():
    return torch.cuda.Stream()


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def cold_then_warm(R, S, held, call, wants, label, *, launch_only=True, kinds=None):
    """the entry once after ``clear_caches()`` and once on the memoised path, both behind a stall; every output against ``wants``"""
    for run in ("cold", "warm"):
        if run == "cold":
            R.clear_caches()
        got, queued = held.run(S, call, launch_only=launch_only and run == "warm")
        if kinds is not None:
            assert kinds(R.last_launch_kinds()), (label, run, R.last_launch_kinds())
        if run == "cold" and launch_only and not queued:
            _LATE_RETURNS.append(label)
        assert len(got) == len(wants)
        for k, (g, w) in enumerate(zip(got, wants)):
            assert same(g, w), (label, run, k, int((g != w).sum()) if g.shape == w.shape else (g.shape, w.shape))


# ----------------------------------------------------------------------------------------------------------------------- the families
def _units_case(O, spec, true, decoy, out_wh, radius, interp, bv, border=0, rot_specs=None, base=None):
    """remap_tensors on n units: (Held, call, wants)"""
    import vr180_convert_amd as V

    dt = {np.uint8: torch.uint8, np.uint16: torch.uint16, np.float32: torch.float32}[true[0].dtype.type]
    held = SO.Held(true, decoy, [((out_wh[1], out_wh[0], true[0].shape[2]), dt)] * len(true))
    t = CS.to_product(spec if base is None else base)
    rots = None if rot_specs is None else [s[1][1] for s in rot_specs]

    def call(srcs, dsts):
        assert V.remap_tensors(t, srcs, dsts, radius=radius, interpolation=interp, boarder_mode=border, boarder_value=bv, rotations=rots) == ["ray"]
        return dsts

    wants = []
    for k, img in enumerate(true):
        xm, ym = O.get_map(spec if rot_specs is None else rot_specs[k], radius=radius, size_input=img.shape[:2], size_output=out_wh)
        wants.append(O.remap(img, xm, ym, interp, border, bv) if img.dtype == np.uint8 else W.remap(img, xm, ym, interp, border, bv))
    return held, call, wants


def test_mirror_pair(V, R, oracle_mod, S):
    _, spec, src_hw, out_wh, radius = PAIR_CASES[0]
    true, decoy = frames(src_hw, 51), frames(src_hw, 71)
    held = SO.Held(true, decoy, [((out_wh[1], 2 * out_wh[0], 3), torch.uint8)])
    t = CS.to_product(spec)

    def call(srcs, dsts):
        return [V.apply_lr_tensors(t, srcs[0], srcs[1], out=dsts[0], size_output=out_wh, interpolation=1, radius=radius, boarder_value=(5, 6, 7))]

    want = oracle_mod.apply_lr(spec, *true, size_output=out_wh, interpolation=1, radius=radius, border_value=(5, 6, 7))
    cold_then_warm(R, S, held, call, [want], "mirror pair", kinds=lambda k: k == ["mirror"])
    _REACHED.add("mirror")


def test_mirror_single_image(V, R, oracle_mod, S):
    _, spec, src_hw, out_wh, radius = PAIR_CASES[0]
    held, call, wants = _units_case(oracle_mod, spec, frames(src_hw, 53)[:1], frames(src_hw, 73)[:1], out_wh, radius, 1, (5, 6, 7))
    cold_then_warm(R, S, held, call, wants, "mirror single", kinds=lambda k: k == ["mirror"])
    _REACHED.add("mirror")


@pytest.mark.parametrize("interp", [2, 4], ids=["bicubic", "lanczos4"])
def test_tile_kxk_pair(V, R, oracle_mod, S, interp):
    spec, (hs, ws), out_wh, radius, bv = C0
    true = [A.noise(np.uint8, hs, ws, 3, 100 + k) for k in range(2)]
    decoy = [A.noise(np.uint8, hs, ws, 3, 110 + k) for k in range(2)]
    held, call, wants = _units_case(oracle_mod, spec, true, decoy, out_wh, radius, interp, bv)
    cold_then_warm(R, S, held, call, wants, f"tile interp {interp}", kinds=lambda k: k == ["tile"])
    _REACHED.add("tile/K4" if interp == 2 else "tile/K8")


@pytest.mark.parametrize("cn", [1, 4], ids=["gray", "bgra"])
def test_cn_kernel(V, R, oracle_mod, S, cn):
    true = [A.noise(np.uint8, 300, 320, cn, 200 + k) for k in range(2)]
    decoy = [A.noise(np.uint8, 300, 320, cn, 210 + k) for k in range(2)]
    held, call, wants = _units_case(oracle_mod, EQUI, true, decoy, (613, 587), 140.0, 1, 77)
    cold_then_warm(R, S, held, call, wants, f"cn {cn}", kinds=lambda k: k == ["cn"])
    _REACHED.add("cn")


def test_lean_batch_of_11_units(V, R, oracle_mod, S):
    (hs, ws), out_wh, spec, radius = LEAN_BATCH["m_table"]
    true = [A.noise(np.uint8, hs, ws, 3, 500 + k) for k in range(11)]
    decoy = [A.noise(np.uint8, hs, ws, 3, 520 + k) for k in range(11)]
    held, call, wants = _units_case(oracle_mod, spec, true, decoy, out_wh, radius, 1, (5, 6, 7))
    cold_then_warm(R, S, held, call, wants, "batch", kinds=lambda k: k == ["batch"])
    _REACHED.add("batch")


def test_rotation_pair_kernel(V, R, oracle_mod, S):
    true, specs = rot_units(3, 600)
    decoy, _ = rot_units(3, 620)
    held, call, wants = _units_case(oracle_mod, None, true, decoy, (448, 448), 80.0, 1, (1, 2, 3), rot_specs=specs, base=ROT_BASE)
    cold_then_warm(R, S, held, call, wants, "rot_pair", kinds=lambda k: k == ["rot_pair"])
    _REACHED.add("rot_pair")


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["uint16", "float32"])
def test_wide_kernel(V, R, oracle_mod, S, dtype):
    g = T.WIDE_PLAIN
    true, decoy = [A.noise(dtype, *g["src_hw"], g["cn"], 6000)], [A.noise(dtype, *g["src_hw"], g["cn"], 6100)]
    held, call, wants = _units_case(oracle_mod, g["spec"], true, decoy, g["out_wh"], g["radius"], 1, T.BV[dtype], border=g["border"])
    cold_then_warm(R, S, held, call, wants, f"wide {np.dtype(dtype).name}", kinds=lambda k: bool(k) and all(x in ("wide", "wide+fixup") for x in k))
    _REACHED.add("wide")


# ----------------------------------------------------------------------------------------------------------------------- the C ABI by ctypes
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["v1c_remap_lut", "v1c_remap_lut_ex"])
def test_remap_lut_entries(R, lib, oracle_mod, S, dtype):
    """the caller's maps are resident, the source is late; 'generic' (k_remap) and 'wide' (k_remap_wide) are these entries' kernels"""
    src, xm, ym, border, bv = T.noise_case(dtype, 3, 1)
    decoy = T.noise_case(dtype, 3, 1, seed=5)[0]
    (hs, ws, cn), (ho, wo), isz = src.shape, xm.shape, src.dtype.itemsize
    dt = torch.uint8 if dtype == np.uint8 else torch.uint16
    held = SO.Held([src], [decoy], [((ho, wo, cn), dt)])
    x_d, y_d = SO.up(xm), SO.up(ym)
    torch.cuda.synchronize()
    cv = R.border_scalar(bv) if dtype == np.uint8 else R.border_scalar_f64(bv)

    def call(srcs, dsts):
        if dtype == np.uint8:
            rc = lib.v1c_remap_lut(0, S.cuda_stream, srcs[0].data_ptr(), hs, ws, ws * cn, cn, dsts[0].data_ptr(), ho, wo, wo * cn, x_d.data_ptr(),
                                   y_d.data_ptr(), wo * 4, 1, border, cv.ctypes.data)
        else:
            rc = lib.v1c_remap_lut_ex(0, S.cuda_stream, srcs[0].data_ptr(), hs, ws, ws * cn * isz, cn, 2, dsts[0].data_ptr(), ho, wo, wo * cn * isz,
                                      x_d.data_ptr(), y_d.data_ptr(), wo * 4, 1, border, cv.ctypes.data)
        assert rc == 0, lib.v1c_last_error()
        return dsts

    want = oracle_mod.remap(src, xm, ym, 1, border, bv) if dtype == np.uint8 else W.remap(src, xm, ym, 1, border, bv)
    for run in range(2):
        got, _ = held.run(S, call, launch_only=run == 1)
        assert same(got[0], want), (run, int((got[0] != want).sum()))
    _REACHED.add("generic" if dtype == np.uint8 else "wide")


def test_remap_fused_one_shot(R, lib, oracle_mod, S):
    """v1c_remap_fused: the first call creates its plan in the library's own cache while the stream is busy, the second finds it"""
    from vr180_convert_amd.chain import lower_for_get_map

    spec, hw, out_wh, radius = T.PLAIN, (96, 104), (88, 72), 48.0
    true, decoy = A.noise(np.uint8, *hw, 3, 700), A.noise(np.uint8, *hw, 3, 701)
    held = SO.Held([true], [decoy], [((out_wh[1], out_wh[0], 3), torch.uint8)])
    chain = lower_for_get_map(CS.to_product(spec), radius=radius, size_input=hw, size_output=out_wh)
    bv = R.border_scalar((9, 8, 7))

    def call(srcs, dsts):
        rc = lib.v1c_remap_fused(0, S.cuda_stream, srcs[0].data_ptr(), hw[0], hw[1], hw[1] * 3, 3, dsts[0].data_ptr(), out_wh[1], out_wh[0],
                                 out_wh[0] * 3, C.byref(chain), 4, 0, bv.ctypes.data)
        assert rc == 0, lib.v1c_last_error()
        return dsts

    xm, ym = oracle_mod.get_map(spec, radius=radius, size_input=hw, size_output=out_wh)
    want = oracle_mod.remap(true, xm, ym, 4, 0, (9, 8, 7))
    for run in ("cold", "warm"):
        got, _ = held.run(S, call, launch_only=run == "warm")
        assert same(got[0], want), (run, int((got[0] != want).sum()))


def test_plan_get_map(V, R, oracle_mod, S):
    """no input to be late: the maps are written behind the stall, read by a consumer on the stream, and overwritten at once"""
    from vr180_convert_amd.chain import lower_for_get_map

    spec, hw, out_wh, radius = T.PLAIN, (192, 208), (176, 144), 96.0
    chain = lower_for_get_map(CS.to_product(spec), radius=radius, size_input=hw, size_output=out_wh)
    plan = R._plan_for(chain, src_hw=hw, dst_wh=out_wh, cn=3, interpolation=1, border_mode=0, border_value=0, device=torch.device("cuda", 0))
    held = SO.Held([], [])
    gx, gy = oracle_mod.get_map(spec, radius=radius, size_input=hw, size_output=out_wh)
    for run in range(2):
        got, _ = held.run(S, lambda srcs, dsts: plan.get_map(), launch_only=run == 1)
        assert_maps_match(got[0], got[1], gx, gy, "get_map behind a stall")


def test_get_radius_async(R, oracle_mod, S):
    true, decoy = discs(300, 170, 158.5), discs(310, 120, 131.5)
    held = SO.Held(true, decoy)
    want = np.array([[oracle_mod.get_radius(im), 0.0] for im in true])
    assert not np.array_equal(want, np.array([[oracle_mod.get_radius(im), 0.0] for im in decoy]))
    for run in range(2):
        got, _ = held.run(S, lambda srcs, dsts: [R.auto_radius_tensor(srcs)], launch_only=run == 1)
        assert np.array_equal(got[0], want), (run, got[0], want)


def test_anaglyph(V, oracle_mod, S):
    true = [A.noise(np.uint8, 72, 100, 3, 800 + k) for k in range(2)]
    decoy = [A.noise(np.uint8, 72, 100, 3, 810 + k) for k in range(2)]
    held = SO.Held(true, decoy)
    want = oracle_mod.anaglyph(*true)
    for run in range(2):
        got, _ = held.run(S, lambda srcs, dsts: [V.anaglyph_tensors(srcs[0], srcs[1])], launch_only=run == 1)
        assert same(got[0], want), run


def test_apply_lr_with_the_radius_found_on_the_device(V, R, oracle_mod, S):
    """radius="auto" without a host round trip: the scan of the late sources and the remap that reads its result are both behind the stall"""
    true, decoy = discs(300, 170, 158.5), discs(320, 131, 140.5)
    held = SO.Held(true, decoy, [((288, 576, 3), torch.uint8)])
    t = CS.to_product(AUTO_SPEC)

    def call(srcs, dsts):
        return [V.apply_lr_tensors(t, srcs[0], srcs[1], out=dsts[0], size_output=(288, 288), interpolation=4, boarder_value=(17, 200, 90),
                                   radius="auto", auto_radius_on_device=True)]

    r = max(oracle_mod.get_radius(im) for im in true)
    assert r != max(oracle_mod.get_radius(im) for im in decoy)
    want = oracle_mod.apply_lr(AUTO_SPEC, *true, size_output=(288, 288), interpolation=4, radius=r, border_value=(17, 200, 90))
    cold_then_warm(R, S, held, call, [want], "kxk-auto", kinds=lambda k: k == ["tile"] and R.last_auto_radius_form() == "device")
    _REACHED.add("kxk-auto")


# ----------------------------------------------------------------------------------------------------------------------- sequences
RING_UNITS = 17  # one more than travels in the kernel arguments: the launch copies its units into a slot of the plan's ring


class RingLaunch:
    """one launch of 17 units with a rotation each, on sources of its own: the buffers, the call and the oracle's outputs"""

    def __init__(self, O, V, index):
        self.V, self.true, self.specs = V, *rot_units(RING_UNITS, 1000 + 40 * index, first=3 * index)
        self.decoy = rot_units(RING_UNITS, 1020 + 40 * index)[0]
        self.late, self.dec = [SO.up(a) for a in self.true], [SO.up(a) for a in self.decoy]
        self.srcs = [d.clone() for d in self.dec]
        self.dsts = [torch.empty((448, 448, 3), dtype=torch.uint8, device="cuda") for _ in self.true]
        self.wants = []
        for img, spec in zip(self.true, self.specs):
            xm, ym = O.get_map(spec, radius=80.0, size_input=(160, 160), size_output=(448, 448))
            self.wants.append(O.remap(img, xm, ym, 1, 0, (1, 2, 3)))
        self.keep = None

    def enqueue(self, late_input, span=None):
        """on the current stream: [the true sources arrive,] the launch [inside ``span``], a consumer, and the buffers are reused at once"""
        if late_input:
            for s, t in zip(self.srcs, self.late):
                s.copy_(t)
        with span if span is not None else contextlib.nullcontext():
            self.V.remap_tensors(CS.to_product(ROT_BASE), self.srcs, self.dsts, radius=80.0, interpolation=1, boarder_value=(1, 2, 3),
                                 rotations=[s[1][1] for s in self.specs])
        self.keep = [d.clone() for d in self.dsts]
        for s, d in zip(self.srcs, self.dec):
            s.copy_(d)
        for d in self.dsts:
            SO.poison(d)

    def check(self, label):
        for k, (g, w) in enumerate(zip(self.keep, self.wants)):
            g = g.cpu().numpy()
            assert same(g, w), (label, k, int((g != w).sum()))


@pytest.fixture(scope="module")
def ring_launches(V, oracle_mod):
    """six launches with the oracle's outputs, computed once and shared by the two ring tests"""
    return [RingLaunch(oracle_mod, V, k) for k in range(6)]


def _warm_ring_plan(V, launches):
    """the plan exists and the decoys are in place before anything is stalled"""
    launches[0].enqueue(late_input=False)
    torch.cuda.synchronize()


def test_six_ring_launches_behind_one_stall(V, R, S, ring_launches):
    """more launches of 17 units than the plan has ring slots (4), each on sources of its own that arrive late, all queued behind ONE
    stall: the fifth and sixth reuse slots whose launches have not run yet"""
    launches = ring_launches
    _warm_ring_plan(V, launches)
    with torch.cuda.stream(S):
        ev = SO.stall(S, 6 * SO.STALL_MS)
        for L in launches:
            L.enqueue(late_input=True)
            assert R.last_launch_kinds() == ["rot_pair"], R.last_launch_kinds()
        queued = not ev.query()
    S.synchronize()
    for k, L in enumerate(launches):
        L.check(f"launch {k}")
    assert queued, "six launch-only calls took longer than the stall: nothing was queued behind it"


def _auto_pair(O, V, true, decoy):
    held = SO.Held(true, decoy, [((288, 288, 3), torch.uint8)] * 2)
    r = max(O.get_radius(im) for im in true)
    xm, ym = O.get_map(AUTO_SPEC, radius=r, size_input=(360, 360), size_output=(288, 288))
    wants = [O.remap(im, xm, ym, 1, 0, (17, 200, 90)) for im in true]
    return held, wants, r


@pytest.fixture(scope="module")
def auto_pairs(V, oracle_mod):
    """two pairs of discs of clearly different radii with the oracle's outputs, shared by the two tests of the dynamic context"""
    a, wa, ra = _auto_pair(oracle_mod, V, discs(300, 170, 158.5), discs(330, 150, 141.5))
    b, wb, rb = _auto_pair(oracle_mod, V, discs(340, 118, 131.5), discs(350, 160, 149.5))
    assert abs(ra - rb) > 20, (ra, rb)
    return a, wa, b, wb


def _enqueue_auto(R, held, late_input=True, span=None):
    """v1c_plan_run_auto_images on the current stream: the launch scans its own (late) sources and rewrites the plan's second context"""
    if late_input:
        for s, t in zip(held.srcs, held.late):
            s.copy_(t)
    with span if span is not None else contextlib.nullcontext():
        R.remap_tensors_auto(CS.to_product(AUTO_SPEC), held.srcs, held.dsts, interpolation=1, boarder_value=(17, 200, 90))
    assert R.last_auto_radius_form() == "device"
    keep = [d.clone() for d in held.dsts]
    for s, d in zip(held.srcs, held.decoy):
        s.copy_(d)
    for d in held.dsts:
        SO.poison(d)
    return keep


def _check_auto(keep, wants, label):
    for k, (g, w) in enumerate(zip(keep, wants)):
        g = g.cpu().numpy()
        assert same(g, w), (label, k, int((g != w).sum()))


def test_two_auto_radius_calls_back_to_back(V, R, S, auto_pairs):
    """two ``v1c_plan_run_auto_images`` calls on one plan with discs of different radii, queued behind one stall: the second call's scan
    rewrites the context the first call's remap reads, and only the stream orders them"""
    a, wa, b, wb = auto_pairs
    _enqueue_auto(R, a, late_input=False)  # (the plan exists)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        ev = SO.stall(S, 2 * SO.STALL_MS)
        ka = _enqueue_auto(R, a)
        kb = _enqueue_auto(R, b)
        queued = not ev.query()
    S.synchronize()
    _check_auto(ka, wa, "first call")
    _check_auto(kb, wb, "second call")
    assert queued


def test_ring_slots_across_two_streams(V, R, ring_launches):
    """Stream A is stalled and carries one 17-unit launch with late sources; stream B, seen to run beside A, then carries five such
    launches of other units on the same plan.  A's call took ring slot s, B's take s + 1, s + 2, s + 3 and then s again: B's FOURTH
    launch lands on the slot of A's launch, which has not run, and ``ring_put`` makes B wait for the slot's event (plan.hip:1011-1012;
    ``ring_done`` records it behind A's remap launch, :1025).  Everything A enqueues -- the upload of its unit records included -- sits
    behind its stall, so the bytes alone cannot show that wait: B, idle, would be done long before A begins.  What shows it is that B is
    SEEN to wait: its first three launches complete while A's stall is still pending, and the span of timing events around the fourth
    covers what is left of the stall (``must_have_waited``).  With the wait deleted that span is a fraction of a millisecond."""
    sa, sb = SO.independent_streams()
    launches = ring_launches
    _warm_ring_plan(V, launches)
    stall_ms = 6 * SO.STALL_MS
    span = SO.Span()
    with torch.cuda.stream(sa):
        t_stall = time.perf_counter()
        ev = SO.stall(sa, stall_ms)
        launches[0].enqueue(late_input=True)
    with torch.cuda.stream(sb):
        for L in launches[1:4]:
            L.enqueue(late_input=True)  # (B is idle: its sources arrive at once, in stream order)
        third = torch.cuda.Event()
        third.record()
        third.synchronize()
        beside = not ev.query()
        launches[4].enqueue(late_input=True, span=span)
        launches[5].enqueue(late_input=True)
        queued = not ev.query()
    sb.synchronize()
    sa.synchronize()
    for k, L in enumerate(launches):
        L.check(f"stream {'A' if k == 0 else 'B'} launch {k}")
    assert beside, "B's first three launches, on slots of their own, did not complete while A was stalled"
    assert queued, "the calls on both streams took longer than A's stall"
    SO.must_have_waited(span, stall_ms, t_stall, "the launch on A's ring slot")


def test_tile_flags_across_two_streams(V, R, oracle_mod):
    """A fix-up pass behind the ray pass, both on the plan's tile-flag words: A stalled with a late source, B on the same plan with another
    source (plan.hip: the wait for flags_ev in front of the ray pass, :1139-1140, its record behind the fix-up pass, :1199).  A's ray
    and fix-up passes sit behind its stall, so B, idle, would never meet A's flag words in between and the bytes cannot show the wait;
    B's call is held to being SEEN to wait for A (``must_have_waited``), which fails the moment the wait is dropped.
    The rectilinear chain of test_one_plan_from_two_threads_and_streams no longer gets a fix-up pass at 300 x 300 -> 320 x 256 (the
    plan proves it unnecessary: the launch reports 'tile', asserted first), so this is the smallest chain of the suite whose launch does
    report one: the rotation into the back hemisphere of tests/chainspecs.py at 256 x 256, asserted too."""
    from vr180_convert_amd.synth import noise_disc

    old = [torch.zeros((300, 300, 3), dtype=torch.uint8, device="cuda")], [torch.empty((256, 320, 3), dtype=torch.uint8, device="cuda")]
    V.remap_tensors(CS.to_product([("equirect_enc", True), ("zoom", 1.4), ("fisheye_dec", "rectilinear")]), *old, radius=40.0, interpolation=1)
    torch.cuda.synchronize()
    assert R.last_launch_kinds() == ["tile"], R.last_launch_kinds()  # (a '+fixup' here: that chain reaches the flags again, use it)

    spec = CS.SMALL_CASES["back_hemisphere"][0]
    t = CS.to_product(spec)
    imgs = [noise_disc(256, 256, 60 + k) for k in range(4)]
    wants = [oracle_mod.apply(spec, [im], size_output=(256, 256), interpolation=1, radius=128.0)[0] for im in imgs[:2]]
    ha, hb = (SO.Held([imgs[k]], [imgs[k + 2]], [((256, 256, 3), torch.uint8)]) for k in range(2))

    def enqueue(h, late, span=None):
        if late:
            h.srcs[0].copy_(h.late[0])
        with span if span is not None else contextlib.nullcontext():
            V.remap_tensors(t, h.srcs, h.dsts, radius=128.0, interpolation=1)
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
    assert kinds_a == kinds_b and kinds_a[0].endswith("+fixup"), (kinds_a, kinds_b)
    for name, keep, want in (("A", ka, wants[0]), ("B", kb, wants[1])):
        g = keep.cpu().numpy()
        assert same(g, want), (name, int((g != want).sum()))
    assert queued
    SO.must_have_waited(span, stall_ms, t_stall, "the ray and fix-up passes on B")


def test_dynamic_context_across_two_streams(V, R, auto_pairs):
    """``v1c_plan_run_auto_images`` on one plan: A stalled, discs of one radius arriving late; B with discs of a clearly different radius
    (plan.hip: the wait for dyn_ev in front of the launch that rewrites the plan-resident context, :1265-1266, its record behind the
    remap, :1291).  A's rewrite of the context sits behind its stall like its remap, so the bytes cannot show the wait: B's call is held
    to being SEEN to wait for A (``must_have_waited``)."""
    a, wa, b, wb = auto_pairs
    sa, sb = SO.independent_streams()
    _enqueue_auto(R, a, late_input=False)
    torch.cuda.synchronize()
    stall_ms, span = 2 * SO.STALL_MS, SO.Span()
    with torch.cuda.stream(sa):
        t_stall = time.perf_counter()
        ev = SO.stall(sa, stall_ms)
        ka = _enqueue_auto(R, a)
    with torch.cuda.stream(sb):
        kb = _enqueue_auto(R, b, span=span)
        queued = not ev.query()
    sb.synchronize()
    sa.synchronize()
    _check_auto(ka, wa, "A")
    _check_auto(kb, wb, "B")
    assert queued
    SO.must_have_waited(span, stall_ms, t_stall, "the auto-radius launch on B")


def test_every_kernel_family_was_reached_behind_a_stall():
    """(the tests above ran: each records the family its launch reported)"""
    assert WANTED <= _REACHED, sorted(WANTED - _REACHED)
    # launch-only entries whose COLD call outlasted the stall: exactly those that create a plan inside the call (v1c_plan_create ends in
    # a device synchronisation, as the header states).  An entry that joins or leaves this set has changed how it blocks.
    assert sorted(set(_LATE_RETURNS)) == COLD_CALLS_THAT_CREATE_A_PLAN, sorted(set(_LATE_RETURNS))
