"""The pair mirror kernels on their plan-time launch records (csrc/tile_device.hpp: MirrorRec), on the GPU: every output byte against
the oracle on the smallest shapes that reach each instantiation -- k_ray_lin3_pair_mirror_seq with and without rest tiles, both table
chains, and the one-eye k_ray_lin3_pair_mirror_raw --, the launch being the mirror launch each time.

The record moves integer arithmetic from every wave to the plan (box decode, fit verdict, units per row, rows per pass, lane ->
(row, unit) of a DMA pass, biased box origins of the tap addresses); source and destination pitches stay with the call, hence the
pitched views.  The record itself against the arithmetic it replaces: tests/test_mirror_record_host.py (no GPU)."""
import numpy as np
import pytest
import torch

import chainspecs as CS

pytestmark = pytest.mark.gpu

EQUI = [("equirect_enc", True), CS.EQUI]                             # m-table chain
POLY = [("equirect_enc", True), ("poly", [0, 1, -0.1]), CS.EQUI]     # w-table chain

# (id, chain, source (h, w), output (w, h), radius)
PAIR_CASES = [
    ("m_300_448_rest", EQUI, (300, 300), (448, 448), 150.0),         # the smallest mirror grid; has rest tiles: REST = 1
    ("w_1000_1028x1024", POLY, (1000, 1000), (1028, 1024), 470.0),   # ragged last tile column
    ("w_120_1024", POLY, (120, 120), (1024, 1024), 60.0),            # boxes of a few rows: many rows per pass, few units per row
    ("m_120_1024", EQUI, (120, 120), (1024, 1024), 60.0),
    # every tile pair of tile rows 0 .. TY / 2 fits the buffers (tests/test_mirror_record_host.py works that out on the host model of the
    # plan's boxes, as for C2's geometry): an empty rest list, the instantiation without the general pair code (REST = 0)
    ("w_1024_rest_free", POLY, (1024, 1024), (1024, 1024), 512.0),
]


@pytest.fixture(scope="module")
def V():
    import vr180_convert_amd as V
    from vr180_convert_amd import _native

    _native.lib()
    assert torch.cuda.is_available()
    return V


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def frames(src_hw, seed):
    from vr180_convert_amd.synth import noise_disc

    left, right = noise_disc(*src_hw, seed), noise_disc(*src_hw, seed + 1)
    left[::9, ::7] = 255
    right[-1, -16:] = 200  # the last bytes are not black: an over-read would show
    return left, right


@pytest.mark.parametrize("name,spec,src_hw,out_wh,radius", PAIR_CASES, ids=[c[0] for c in PAIR_CASES])
def test_pairs_on_the_launch_record(V, oracle_mod, dev, name, spec, src_hw, out_wh, radius):
    from vr180_convert_amd import remapper

    left, right = frames(src_hw, 51)
    want = oracle_mod.apply_lr(spec, left, right, size_output=out_wh, interpolation=1, radius=radius, border_value=(5, 6, 7))
    got = V.apply_lr_tensors(CS.to_product(spec), torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev), size_output=out_wh,
                             interpolation=1, radius=radius, boarder_value=(5, 6, 7)).cpu().numpy()
    assert remapper.last_launch_kinds() == ["mirror"], remapper.last_launch_kinds()
    assert np.array_equal(got, want), (name, int((got != want).sum()))


@pytest.mark.parametrize("name,spec,src_hw,out_wh,radius", PAIR_CASES[:2], ids=[c[0] for c in PAIR_CASES[:2]])
def test_pairs_with_pitched_sources_and_destination(V, oracle_mod, dev, name, spec, src_hw, out_wh, radius):
    """Sources that are column slices of one wider frame (pitch != 3 * width, rows still dword-aligned) and a destination that is a
    window of a larger buffer: the products with the pitches are the part of the prologue that stayed in the kernel."""
    from vr180_convert_amd import remapper
    from vr180_convert_amd.synth import noise_disc

    h, w = src_hw
    wide = noise_disc(h, 2 * w + 24, 61)
    wide[::5, ::3] = 250
    wide[-1, -16:] = 200
    l_np, r_np = wide[:, 4:4 + w], wide[:, w + 16:2 * w + 16]
    want = oracle_mod.apply_lr(spec, np.ascontiguousarray(l_np), np.ascontiguousarray(r_np), size_output=out_wh, interpolation=1,
                               radius=radius, border_value=(5, 6, 7))
    fr = torch.from_numpy(wide).to(dev)
    W, H = out_wh
    big = torch.full((H + 3, 2 * W + 8, 3), 99, dtype=torch.uint8, device=dev)
    sbs = big[2:2 + H, 4:4 + 2 * W]  # (12 bytes in: rows stay dword-aligned, pitch = 3 * (2 W + 8))
    V.apply_lr_tensors(CS.to_product(spec), fr[:, 4:4 + w], fr[:, w + 16:2 * w + 16], out=sbs, size_output=out_wh, interpolation=1,
                       radius=radius, boarder_value=(5, 6, 7))
    assert remapper.last_launch_kinds() == ["mirror"], remapper.last_launch_kinds()
    got = big.cpu().numpy()
    assert np.array_equal(got[2:2 + H, 4:4 + 2 * W], want), (name, int((got[2:2 + H, 4:4 + 2 * W] != want).sum()))
    frame = np.ones(got.shape[:2], bool)
    frame[2:2 + H, 4:4 + 2 * W] = False
    assert (got[frame] == 99).all()  # nothing written around the window


@pytest.mark.parametrize("name,spec,src_hw,out_wh,radius", PAIR_CASES[:2], ids=[c[0] for c in PAIR_CASES[:2]])
def test_one_image_on_the_launch_record(V, oracle_mod, dev, name, spec, src_hw, out_wh, radius):
    """apply() of ONE image: the one-eye instantiation of k_ray_lin3_pair_mirror_raw reads the same records (its own fit bit), from a
    pitched source view into a pitched destination."""
    from vr180_convert_amd import remapper
    from vr180_convert_amd.synth import noise_disc

    h, w = src_hw
    wide = noise_disc(h, w + 8, 71)
    wide[::7, ::5] = 255
    img = wide[:, 4:4 + w]
    want = oracle_mod.apply(spec, [np.ascontiguousarray(img)], size_output=out_wh, interpolation=1, radius=radius, border_value=(5, 6, 7))[0]
    W, H = out_wh
    big = torch.full((H, W + 4, 3), 99, dtype=torch.uint8, device=dev)
    dst = big[:, 4:]
    V.remap_tensors(CS.to_product(spec), [torch.from_numpy(wide).to(dev)[:, 4:4 + w]], [dst], radius=radius, interpolation=1,
                    boarder_value=(5, 6, 7))
    assert remapper.last_launch_kinds() == ["mirror"], remapper.last_launch_kinds()
    got = big.cpu().numpy()
    assert np.array_equal(got[:, 4:], want), (name, int((got[:, 4:] != want).sum()))
    assert (got[:, :4] == 99).all()


@pytest.mark.parametrize("env", [{"V1C_MIRROR_REC": "0"}, {}], ids=["V1C_MIRROR_REC=0", "tuning default"])
def test_tuning_twin_keeps_the_box_prologue(env):
    """The -DV1C_TUNING twin of the library: V1C_MIRROR_REC=0 selects the kernels that decode the box pair in every wave (the A/B
    partners of profiles/mirror_record/), the default the record-reading ones; both give the oracle's bytes, with and without rest
    tiles, pairs and one image (tests/mirror_record_probe.py in a subprocess: the switch is read once per process)."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    from vr180_convert_amd import _native

    tuning = _native.LIB_PATH.with_name("libvr180remap_tuning.so")
    assert tuning.exists(), "built by __graft_entry__.build()"
    probe = Path(__file__).with_name("mirror_record_probe.py")
    r = subprocess.run([sys.executable, str(probe)], env={**os.environ, **env, "V1C_LIB": str(tuning)}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
