"""The pair mirror kernel on a plan's tap table (csrc/tap_table.hpp, k_ray_lin3_pair_mirror_seq_tab), on the GPU: every output byte
against the oracle, each case asserting that its plan holds a table (``remapper.last_tap_table_bytes()``) or holds none.

A pair plan without rest tiles keeps the fixed-point tap coordinates of every lane, filled once at creation by the seq kernel's own
coordinate code; its launches read 12 bytes per lane where k_ray_lin3_pair_mirror_seq<., 0> evaluates the map.  What can go wrong is
therefore: the fill against the kernel's coordinates (both table chains: the w-table POLY chain and the m-table EQUI chain), the
entry's way through LDS, what stayed with the call (pitches, windows, streams, captured launches), a table outliving or missing its
plan (a changed radius is a new plan with a new table), and the rule that a plan with rest tiles holds none.  Shapes: the rest-free
case of tests/test_gpu_mirror_record.py (16 x 33 tile pairs) and, for EQUI, the smallest mirror grid of that file (300 -> 448) with the
radius pulled inside the source, 146 instead of 150: on the host model of the plan's boxes (tests/test_mirror_record_host.py's
model_boxes) every one of its 105 tile pairs then fits, and smaller EQUI grids (120 -> 128, 200 -> 192) do not take the mirror launch
at all.  The oracle's results are computed once per module."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import chainspecs as CS

pytestmark = pytest.mark.gpu

EQUI = [("equirect_enc", True), CS.EQUI]                             # m-table chain
POLY = [("equirect_enc", True), ("poly", [0, 1, -0.1]), CS.EQUI]     # w-table chain
BORDER = (5, 6, 7)
FREE = (POLY, (1024, 1024), (1024, 1024))                            # w_1024_rest_free of tests/test_gpu_mirror_record.py
EQUI_FREE = (EQUI, (300, 300), (448, 448), 146.0)                    # the smallest mirror grid (m_300_448_rest) with the circle inside the source: rest-free
ENTRY_BYTES = 12


def table_bytes(out_wh):
    """one entry per lane of the tile pairs of tile rows 0 .. TY / 2 (64 x 16 tiles, 256 lanes)"""
    w, h = out_wh
    return ((w + 63) // 64) * ((h + 15) // 16 // 2 + 1) * 256 * ENTRY_BYTES


@pytest.fixture(scope="module")
def V():
    import vr180_convert_amd as V
    from vr180_convert_amd import _native

    _native.lib()
    assert torch.cuda.is_available()
    return V


@pytest.fixture(scope="module")
def R():
    from vr180_convert_amd import remapper

    return remapper


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def frames(src_hw, seed):
    from vr180_convert_amd.synth import noise_disc

    left, right = noise_disc(*src_hw, seed), noise_disc(*src_hw, seed + 1)
    left[::9, ::7] = 255
    right[-1, -16:] = 200  # the last bytes are not black: an over-read would show
    return left, right


@pytest.fixture(scope="module")
def ref(oracle_mod):
    """pixels A and B of the rest-free geometry and the oracle's side-by-side results, computed once and never written to"""
    spec, src_hw, out_wh = FREE
    out = {"A": frames(src_hw, 51), "B": frames(src_hw, 61)}
    for key, px, radius in (("A512", "A", 512.0), ("B512", "B", 512.0), ("A500", "A", 500.0)):
        out[key] = oracle_mod.apply_lr(spec, *out[px], size_output=out_wh, interpolation=1, radius=radius, border_value=BORDER)
        out[key].setflags(write=False)
    return out


def run_pair(V, dev, spec, left, right, out_wh, radius, out=None):
    return V.apply_lr_tensors(CS.to_product(spec), left if torch.is_tensor(left) else torch.from_numpy(left).to(dev),
                              right if torch.is_tensor(right) else torch.from_numpy(right).to(dev), out=out, size_output=out_wh,
                              interpolation=1, radius=radius, boarder_value=BORDER)


def pitched(dev, left, right, out_wh):
    """column slices of one wider frame as sources and a window of a larger buffer, filled with 99, as destination"""
    h, w = left.shape[:2]
    wide = np.full((h, 2 * w + 24, 3), 17, np.uint8)
    wide[:, 4:4 + w], wide[:, w + 16:2 * w + 16] = left, right
    fr = torch.from_numpy(wide).to(dev)
    W, H = out_wh
    big = torch.full((H + 3, 2 * W + 8, 3), 99, dtype=torch.uint8, device=dev)
    return fr[:, 4:4 + w], fr[:, w + 16:2 * w + 16], big, big[2:2 + H, 4:4 + 2 * W]


def check_window(big, out_wh, want, what):
    W, H = out_wh
    got = big.cpu().numpy()
    assert np.array_equal(got[2:2 + H, 4:4 + 2 * W], want), (what, int((got[2:2 + H, 4:4 + 2 * W] != want).sum()))
    guard = np.ones(got.shape[:2], bool)
    guard[2:2 + H, 4:4 + 2 * W] = False
    assert (got[guard] == 99).all(), what  # nothing written around the window


def test_in_use_on_the_rest_free_poly_plan(V, R, dev, ref):
    spec, src_hw, out_wh = FREE
    got = run_pair(V, dev, spec, *ref["A"], out_wh, 512.0).cpu().numpy()
    assert R.last_launch_kinds() == ["mirror"], R.last_launch_kinds()
    assert R.last_tap_table_bytes() == [table_bytes(out_wh)] == [16 * 33 * 3072]
    assert np.array_equal(got, ref["A512"]), int((got != ref["A512"]).sum())


def test_in_use_on_a_rest_free_equi_plan(V, R, oracle_mod, dev):
    """the m-table chain: the fill runs the other lane_coords instantiations (VAR_W = 0; polynomials in m where the plan flags them)"""
    spec, src_hw, out_wh, radius = EQUI_FREE
    left, right = frames(src_hw, 71)
    want = oracle_mod.apply_lr(spec, left, right, size_output=out_wh, interpolation=1, radius=radius, border_value=BORDER)
    got = run_pair(V, dev, spec, left, right, out_wh, radius).cpu().numpy()
    assert R.last_launch_kinds() == ["mirror"], R.last_launch_kinds()
    assert R.last_tap_table_bytes() == [table_bytes(out_wh)] == [7 * 15 * 3072]
    assert np.array_equal(got, want), int((got != want).sum())


def test_in_use_with_pitched_sources_and_a_destination_window(V, R, dev, ref):
    spec, src_hw, out_wh = FREE
    l, r, big, win = pitched(dev, *ref["A"], out_wh)
    run_pair(V, dev, spec, l, r, out_wh, 512.0, out=win)
    assert R.last_launch_kinds() == ["mirror"] and R.last_tap_table_bytes() == [table_bytes(out_wh)]
    check_window(big, out_wh, ref["A512"], "pitched")


def test_two_calls_on_one_plan_with_different_pixels_and_pitches(V, R, dev, ref):
    """the table belongs to the plan, pixels and pitches to the call: a contiguous call, then other pixels through pitched views"""
    spec, src_hw, out_wh = FREE
    R.clear_caches()
    first = run_pair(V, dev, spec, *ref["A"], out_wh, 512.0)
    assert R.last_tap_table_bytes() == [table_bytes(out_wh)]
    n_plans = len(R._PLANS)
    l, r, big, win = pitched(dev, *ref["B"], out_wh)
    run_pair(V, dev, spec, l, r, out_wh, 512.0, out=win)
    assert len(R._PLANS) == n_plans == 1, "the second call must reuse the plan"
    assert R.last_launch_kinds() == ["mirror"] and R.last_tap_table_bytes() == [table_bytes(out_wh)]
    check_window(big, out_wh, ref["B512"], "second call")
    assert np.array_equal(first.cpu().numpy(), ref["A512"])


def test_in_use_on_a_busy_side_stream_right_after_plan_creation(V, R, dev, ref):
    """The table is filled at creation, not in stream order of the first launch: a launch queued on a stalled side stream directly behind
    the call that created the plan must find it complete, and must itself stay behind the stream's earlier work (the true pixels
    only arrive on that stream, behind the stall)."""
    import stream_order as SO

    spec, src_hw, out_wh = FREE
    R.clear_caches()
    decoy_l, decoy_r = (torch.from_numpy(x).to(dev) for x in ref["B"])
    true_l, true_r = (torch.from_numpy(x).to(dev) for x in ref["A"])
    src_l, src_r = decoy_l.clone(), decoy_r.clone()
    out = torch.empty((out_wh[1], 2 * out_wh[0], 3), dtype=torch.uint8, device=dev)
    run_pair(V, dev, spec, src_l, src_r, out_wh, 512.0, out=out)  # creates the plan (and its table); the decoy's result
    assert R.last_tap_table_bytes() == [table_bytes(out_wh)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    ev = SO.stall(s, 3 * SO.STALL_MS)  # (two copies and the call are queued behind it)
    with torch.cuda.stream(s):
        src_l.copy_(true_l), src_r.copy_(true_r)
        run_pair(V, dev, spec, src_l, src_r, out_wh, 512.0, out=out)
        launched_behind_the_stall = not ev.query()
        keep = out.clone()
        src_l.copy_(decoy_l), src_r.copy_(decoy_r), out.fill_(SO.POISON)
    s.synchronize()
    assert launched_behind_the_stall, "the call returned only after the stall: it synchronised"
    assert R.last_launch_kinds() == ["mirror"] and R.last_tap_table_bytes() == [table_bytes(out_wh)]
    assert np.array_equal(keep.cpu().numpy(), ref["A512"]), int((keep.cpu().numpy() != ref["A512"]).sum())


def test_in_use_in_a_captured_launch_replayed_on_new_pixels(V, R, dev, ref):
    spec, src_hw, out_wh = FREE
    src_l, src_r = (torch.from_numpy(x).to(dev) for x in ref["A"])
    out = torch.empty((out_wh[1], 2 * out_wh[0], 3), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up on the capture stream: the plan exists before capture starts
        run_pair(V, dev, spec, src_l, src_r, out_wh, 512.0, out=out)
    torch.cuda.synchronize()
    assert R.last_tap_table_bytes() == [table_bytes(out_wh)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run_pair(V, dev, spec, src_l, src_r, out_wh, 512.0, out=out)
    assert R.last_launch_kinds() == ["mirror"] and R.last_tap_table_bytes() == [table_bytes(out_wh)]
    for px, key in (("B", "B512"), ("A", "A512")):
        src_l.copy_(torch.from_numpy(ref[px][0]).to(dev)), src_r.copy_(torch.from_numpy(ref[px][1]).to(dev))
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), ref[key]), (px, int((out.cpu().numpy() != ref[key]).sum()))


def test_a_changed_radius_is_a_new_plan_with_a_new_table(V, R, dev, ref):
    spec, src_hw, out_wh = FREE
    R.clear_caches()
    a = run_pair(V, dev, spec, *ref["A"], out_wh, 512.0).cpu().numpy()
    assert R.last_tap_table_bytes() == [table_bytes(out_wh)] and len(R._PLANS) == 1
    b = run_pair(V, dev, spec, *ref["A"], out_wh, 500.0).cpu().numpy()
    assert len(R._PLANS) == 2, "another radius is another map: a plan of its own"
    assert R.last_launch_kinds() == ["mirror"] and R.last_tap_table_bytes() == [table_bytes(out_wh)]
    assert np.array_equal(a, ref["A512"]) and np.array_equal(b, ref["A500"]), (int((a != ref["A512"]).sum()), int((b != ref["A500"]).sum()))
    # ... and the first plan still serves its own radius from its own table
    again = run_pair(V, dev, spec, *ref["A"], out_wh, 512.0).cpu().numpy()
    assert len(R._PLANS) == 2 and np.array_equal(again, ref["A512"])


def test_not_in_use_on_a_plan_with_rest_tiles(V, R, oracle_mod, dev):
    """m_300_448_rest of tests/test_gpu_mirror_record.py: rest tiles, so no table and the kernel that evaluates the map"""
    spec, src_hw, out_wh, radius = EQUI, (300, 300), (448, 448), 150.0
    left, right = frames(src_hw, 51)
    want = oracle_mod.apply_lr(spec, left, right, size_output=out_wh, interpolation=1, radius=radius, border_value=BORDER)
    got = run_pair(V, dev, spec, left, right, out_wh, radius).cpu().numpy()
    assert R.last_launch_kinds() == ["mirror"], R.last_launch_kinds()
    assert R.last_tap_table_bytes() == [0]
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("env", [{"V1C_MIRROR_TAB": "0"}, {}], ids=["V1C_MIRROR_TAB=0", "tuning default"])
def test_tuning_twin_has_the_computing_kernel_as_ab_partner(env):
    """The -DV1C_TUNING twin: V1C_MIRROR_TAB=0 launches k_ray_lin3_pair_mirror_seq<., 0> although the plan holds a table (the A/B partner
    of profiles/tap_table/), the default the table kernel; both give the oracle's bytes on both table chains
    (tests/tap_table_probe.py in a subprocess: the switch is read once per process)."""
    from vr180_convert_amd import _native

    tuning = _native.LIB_PATH.with_name("libvr180remap_tuning.so")
    assert tuning.exists(), "built by __graft_entry__.build()"
    probe = Path(__file__).with_name("tap_table_probe.py")
    r = subprocess.run([sys.executable, str(probe)], env={**os.environ, **env, "V1C_LIB": str(tuning)}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
