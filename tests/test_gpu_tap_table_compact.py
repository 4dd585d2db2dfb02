"""The compact (8-byte) entry of the pair mirror kernel's tap table (csrc/tap_table.hpp: TapEntry8, k_ray_lin3_pair_mirror_seq_tab8),
on the GPU: every output byte against the oracle, each case asserting the size of its plan's table (``remapper.last_tap_table_bytes()``).

A rest-free pair plan takes the compact entry when its 12-byte table would pass 8 MiB (plan.hip: kTapCompactMinBytes) and the 12-byte
entry otherwise.  What can go wrong beyond tests/test_gpu_tap_table.py is therefore: the fill's compact encoding against the kernel's
decode on both table chains (forced with V1C_TAP_FORM=8 in the tuning twin on that file's two chains), the 8-byte entry's way through
LDS, the K that the launch record carries against the K the fill used, and the rule itself on either side of the threshold.  Shapes:
the smallest rest-free pair above the threshold, POLY 2048 -> 2688 at radius 1024 (42 x 85 tile pairs: 10 967 040 B in the 12-byte
form, 7 311 360 B compact) and, just under it, 2048 -> 2304 (36 x 73: 8 073 216 B, 12-byte entries); on the host box model of
tests/test_mirror_record_host.py (model_boxes, raw_passes, mirror_raw_fit restated) neither has a rest tile, nor has 2688 at radius 1000,
while the EQUI chain 2048 -> 2688 at radius 1024 leaves 50 tile pairs to the general code.  The oracle's results are computed once per
module."""
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
SRC_HW = (2048, 2048)
OVER = (2688, 2688)     # 12-byte table 10 967 040 B > 8 MiB: compact
UNDER = (2304, 2304)    # 8 073 216 B < 8 MiB: 12-byte entries


def table_bytes(out_wh, entry_bytes):
    """one entry per lane of the tile pairs of tile rows 0 .. TY / 2 (64 x 16 tiles, 256 lanes)"""
    w, h = out_wh
    return ((w + 63) // 64) * ((h + 15) // 16 // 2 + 1) * 256 * entry_bytes


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
    """pixels A and B and the oracle's side-by-side results, computed once and never written to"""
    out = {"A": frames(SRC_HW, 51), "B": frames(SRC_HW, 61)}
    for key, spec, px, out_wh, radius in (("A1024", POLY, "A", OVER, 1024.0), ("B1024", POLY, "B", OVER, 1024.0), ("A1000", POLY, "A", OVER, 1000.0),
                                          ("A_under", POLY, "A", UNDER, 1024.0), ("A_equi", EQUI, "A", OVER, 1024.0)):
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


def test_tuning_twin_runs_both_table_chains_in_the_compact_form():
    """The -DV1C_TUNING twin with V1C_TAP_FORM=8: the two chains of tests/test_gpu_tap_table.py (the w-table and the m-table fill) keep
    8-byte entries at sizes far below the threshold and give the oracle's bytes (tests/tap_table_compact_probe.py in a subprocess: the
    switch belongs to the process)."""
    from vr180_convert_amd import _native

    tuning = _native.LIB_PATH.with_name("libvr180remap_tuning.so")
    assert tuning.exists(), "built by __graft_entry__.build()"
    probe = Path(__file__).with_name("tap_table_compact_probe.py")
    r = subprocess.run([sys.executable, str(probe)], env={**os.environ, "V1C_TAP_FORM": "8", "V1C_LIB": str(tuning)}, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]


def test_compact_above_the_threshold(V, R, dev, ref):
    """the product, no environment: the smallest rest-free pair whose 12-byte table passes 8 MiB"""
    R.clear_caches()
    got = run_pair(V, dev, POLY, *ref["A"], OVER, 1024.0).cpu().numpy()
    assert R.last_launch_kinds() == ["mirror"], R.last_launch_kinds()
    assert table_bytes(OVER, 12) == 42 * 85 * 3072 == 10_967_040 > 8 << 20
    assert R.last_tap_table_bytes() == [table_bytes(OVER, 8)] == [7_311_360] and R.last_tap_entry_bytes() == [8]
    assert np.array_equal(got, ref["A1024"]), int((got != ref["A1024"]).sum())
    # pitched sources and a destination window on the same plan
    n_plans = len(R._PLANS)
    l, r, big, win = pitched(dev, *ref["A"], OVER)
    run_pair(V, dev, POLY, l, r, OVER, 1024.0, out=win)
    assert len(R._PLANS) == n_plans == 1
    assert R.last_launch_kinds() == ["mirror"] and R.last_tap_table_bytes() == [7_311_360]
    check_window(big, OVER, ref["A1024"], "pitched")
    # a second call with other pixels, contiguous this time: the table belongs to the plan, the pixels to the call
    got = run_pair(V, dev, POLY, *ref["B"], OVER, 1024.0).cpu().numpy()
    assert len(R._PLANS) == 1, "the call must reuse the plan"
    assert R.last_launch_kinds() == ["mirror"] and R.last_tap_table_bytes() == [7_311_360]
    assert np.array_equal(got, ref["B1024"]), int((got != ref["B1024"]).sum())


def test_twelve_byte_entries_just_under_the_threshold(V, R, dev, ref):
    got = run_pair(V, dev, POLY, *ref["A"], UNDER, 1024.0).cpu().numpy()
    assert R.last_launch_kinds() == ["mirror"], R.last_launch_kinds()
    assert R.last_tap_table_bytes() == [table_bytes(UNDER, 12)] == [36 * 73 * 3072] == [8_073_216] and 8_073_216 < 8 << 20
    assert R.last_tap_entry_bytes() == [12]
    assert np.array_equal(got, ref["A_under"]), int((got != ref["A_under"]).sum())


def test_a_changed_radius_is_a_new_plan_with_a_compact_table_of_its_own(V, R, dev, ref):
    R.clear_caches()
    a = run_pair(V, dev, POLY, *ref["A"], OVER, 1024.0).cpu().numpy()
    assert R.last_tap_table_bytes() == [7_311_360] and len(R._PLANS) == 1
    b = run_pair(V, dev, POLY, *ref["A"], OVER, 1000.0).cpu().numpy()
    assert len(R._PLANS) == 2, "another radius is another map: a plan of its own"
    assert R.last_launch_kinds() == ["mirror"] and R.last_tap_table_bytes() == [7_311_360] and R.last_tap_entry_bytes() == [8]
    assert np.array_equal(a, ref["A1024"]) and np.array_equal(b, ref["A1000"]), (int((a != ref["A1024"]).sum()), int((b != ref["A1000"]).sum()))
    again = run_pair(V, dev, POLY, *ref["A"], OVER, 1024.0).cpu().numpy()  # the first plan still serves its radius from its own table
    assert len(R._PLANS) == 2 and np.array_equal(again, ref["A1024"])


def test_no_table_on_a_plan_with_rest_tiles_in_the_compact_range(V, R, dev, ref):
    """the EQUI chain at the same size: the source's rim leaves tile pairs to the general code, so the plan holds no table in either form"""
    got = run_pair(V, dev, EQUI, *ref["A"], OVER, 1024.0).cpu().numpy()
    assert R.last_launch_kinds() == ["mirror"], R.last_launch_kinds()
    assert R.last_tap_table_bytes() == [0] and R.last_tap_entry_bytes() == [0]
    assert np.array_equal(got, ref["A_equi"]), int((got != ref["A_equi"]).sum())
