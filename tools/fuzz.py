#!/usr/bin/env python3
"""Differential fuzz on the GPU: random chains / sizes / flags through the product (C ABI, HIP kernels) against the CPU oracle,
byte for byte, for a bounded time.  Wider than the seeded sweeps of tests/test_gpu_parity.py (those are the regression net; this
is the search): chains drawn from a grammar over every lowered stage, sizes from 1 px to a few thousand (several tile rows, XCD
strips, rest lists, the unit ring), cn 1 / 3 / 4, every interpolation and border mode incl. BORDER_TRANSPARENT, pitched source
and destination views (dword-aligned or not), per-unit rotations, apply_lr pairs; a share of the cases (--lut) runs cv2.remap alone
(v1c_remap_lut) on random float32 maps sprinkled with NaN, infinities, 2^15 / 2^26 / 2^31-scale values and ties of the 1/32 grid.

    python3 tools/fuzz.py [--seconds 300] [--seed 1] [--big 0.15] [--lut 0.15] [--hot 0.3] [--gen2 0] [--api 0.1] [--auto 0.06] [--fused 0.06] [--log gpurun_out/fuzz.log]
                          [--wide 0] [--png 0] [--jpeg 0] [--feat 0] [--jpegdec 0] [--jpegbatch 0] [--jpegopt 0] [--jpegprog 0] [--jpegxc 0] [--jpegxf 0] [--jpegdmg 0] [--jpegodd 0] [--circle 0] [--colormatch 0] [--vignette 0] [--cases N]

--wide P: that share of the cases has uint16 or float32 pixels (k_remap_wide): the chain cases above -- same grammar, views, batches, pairs,
per-unit rotations, graph replays and the same three masks, counted in the same counters -- and the LUT cases (v1c_remap_lut_ex, nothing left
out), against tests/wide_ref.py's restatement of cv2's float-weight remap on the oracle's map; a third of the float32 sources hold denormals,
values next to FLT_MAX, signed zeros, infinities and NaN.  Outputs stay under 640 px (320 px for the 4 x 4 and 8 x 8 kernels) so that the NumPy
restatement takes seconds.  A wide chain case whose masks leave out more than 5 % of its pixels is checked like any other but does not count
towards the run's case total (the summary line says how many).  --png P: that share goes through the device PNG encoder
(encode_png_tensor) -- a remap result as it lies on the device, or a synthetic image of tests/png_cases.py's generators (run planes across the
kernels' 64-lane steps, 256-byte segments and 64-segment groups, noise, Fibonacci frequencies; gray / BGR / BGRA, 8- and 16-bit) in a random
view with a random band height and either filter -- against tests/png_ref.py's file, byte for byte.  --jpeg P: that share goes through the device JPEG encoder (encode_jpeg_tensor) -- a remap result or a
random image in a random view, any quality, either subsampling, a random restart interval -- against tests/jpg_ref.py's file, byte for
byte.  --jpegbatch P: that share goes through the batched device JPEG encoder (encode_jpeg_tensors) -- lists of 1 to 12 random images up to 96 x 96, each with its own parameters -- against the single calls and tests/jpg_ref.py.  --jpegopt P: that share goes through the device JPEG encoder with optimised Huffman tables (optimize=True) -- lists of 1 to 8 random images up to 160 x 160 that mix optimising and plain images -- against tests/jpg_opt_ref.py and the single calls.  --jpegdec P: that share goes through the device JPEG decoder (decode_jpeg_tensor) -- a random image up to 96 x 96 written by Pillow or
by tests/jpg_ref.py with random sampling, quality, restart setting and optimised tables, at a random subsequence size -- against
tests/jpgdec_ref.py's pixels, byte for byte.  --feat P: that share goes through the feature
pipeline of --automatch devfm (features.detect / features.match) against tests/feat_ref.py, keypoints, descriptors and matches equal: images of
six kinds (noise discs, noise, low contrast, polygons and blobs on a gradient, rendered sphere scenes, flat) of 40 ... 700 px in random views,
scale, radius, margin, threshold, cell, per_cell and the cap drawn off their defaults, the matcher on the descriptors of two detects or on random
sets of 0 ... 20000 descriptors with planted copies, duplicates and ties.  A case that v1c_feat_detect refuses (working image under 33 x 33, empty
circle) where feat_ref.refusal predicts it is correct and not counted (the summary line says how many).  --jpegprog P: that share goes through the device decoder of progressive JPEG files
(decode_jpeg_tensor(progressive=True)) -- Pillow's progressive files and tests/jpgprog_cases.py's writer with random legal scan scripts --
against tests/jpgprog_ref.py: pixels, scans and the rounds of every scan.  --jpegxf P: that share goes through the lossless JPEG composer (compose_regions) -- one to four random files of one kind up to 96 x 96 and one or two outputs of strips under random codes -- against tests/jpgxf_ref.py, byte for byte; a composition both sides refuse alike counts as agreement (the summary line says how many).  --jpegdmg P: that share goes through the device JPEG decoders (v1c_jpeg_decode,
v1c_jpeg_prog_decode) with a DAMAGED scan -- a file as --jpegdec / --jpegprog draw it, one random damage of tests/jpgdmg_cases.py's kinds (a bit
flipped, a byte replaced, 1-3 bytes deleted or inserted, two restart segments exchanged, the scan filled) inside the entropy-coded bytes of one
scan, a random subsequence size -- against the restatement's verdict: the code, the smallest bad bit and its scan, the rounds, and the pixels of
damage that is still a legal stream (the summary line says how many cases were refused by the last pass, decoded, or left to the parse).  --jpegodd P: that share goes through the same two entries with a LEGAL file of unusual structure (drawn Huffman code shapes
and table slots, 16-bit quantisation tables, component ids, segment orders, fill bytes, DRI oddities) or with ONE damage in a marker
segment of a small supported file (tests/jpgodd_cases.py), against the restatement: the parse's class, then the verdict as for --jpegdmg
(the summary line says how many were refused as predicted).  --circle P: that share goes through the image-circle fit
(v1c_fit_circle: random discs, clips, wedges, noise, pixel types, channel counts, views and parameters) against tests/circle_ref.py --
rim points, selection flags and counts equal, floats within 1e-9 px -- and, for a part of them, through apply() / apply_lr_tensors()
with random off-centre center= values against oracle.remap of the host NumPy chain's map with those centres.  --colormatch P: that
share goes through the colour match of two eyes (color_match_luts_tensor + apply_luts_tensor: random sizes with odd widths, channel
counts, pitches, offsets, halves of a side-by-side buffer, modes, references, parameters off the defaults, in place and out of place,
noise, flat frames, gradients and discs on black whose surrounds differ) against tests/colormatch_ref.py, byte for byte: histograms,
tables, report, result and every byte of the buffer around the eyes.  --vignette P: that share goes through the vignetting correction
(vignette_rings_tensor + apply_vignette_tensor: random sizes, channel counts, uint8 / uint16, pitches, offsets, the right half of a
side-by-side buffer, centres inside and up to one frame size outside the frame, radii from 1 px up, coefficients, gammas, ring counts,
masks, in place and out of place) against tests/vignette_ref.py, byte for byte: the ring record, the result and every byte of the
buffer around the image.  These shares come off
the top of the case draw: with all of them at 0 every earlier seed replays as it ran.

Round 5 added to the grammar: hot shapes of the chains that left the interpreter (planar fisheye -> fisheye, is_latitude_y=False, a
rotation behind radial stages), outputs of 64 ... 416 px, launches recorded into a graph and replayed, radius='auto' with the radius on
the device (--auto) and v1c_remap_fused through raw ctypes (--fused); --gen2: chains forced into general mode 2 (radial stages / zooms in front
of a rotation, lanes split between the tile kernel and the fix-up pass: what case 1974 of seed 34 was).  tools/fuzz_cpu.py is the GPU-less half.

Ill-conditioned pixels are left out and counted: where the chain amplifies a perturbation of the output position by 1e6 or more
(measured on the oracle's fp64 map, `ill_conditioned`), the last bits of every intermediate -- they differ between glibc and the
device's libm, and with fused multiply-adds -- decide the pixel.  Two kinds turned up: poles of a rectilinear projection (tan(theta)
at or beside 90 degrees: a coordinate of 1e6 ... 1e19 px, the other one the ratio of two rounding residues of pi / 2; seed 1, many
cases; seed 2 case 1423) and stacked polynomial stages that take the angle to 1e12 rad before a decoder takes its tangent (seed 5
case 1534: 5.6 % of the pixels).  The product's per-pixel code compiled for the HOST equals the oracle on them up to a handful of
pixels (tests/test_host_emul.py's emulation): it is the arithmetic environment, not the algorithm.  Under the border modes that read
source pixels far outside (REPLICATE, REFLECT, WRAP, REFLECT_101) pixels with a map coordinate of magnitude >= 2^20 are left out as
well (cv2 itself saturates integer coordinates at 2^15).  A unit that still differs is checked for float32 rounding ties (float32_ties:
measure zero, counted apart).

Every mismatch is printed as a self-contained case description (seed + case number reproduce it: `--seed S --only N`); exit code 1
if there was one.  The oracle is test infrastructure: this tool is not part of the product.
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import chainspecs as CS  # noqa: E402
import wide_ref as W  # noqa: E402
import vr180_convert_amd as V  # noqa: E402
from oracle import oracle as O  # noqa: E402

MODELS = ["rectilinear", "stereographic", "equidistant", "equisolid", "orthographic"]


def rand_rot(rng, big: bool):
    from vr180_convert_amd.quat import as_rotation_matrix, from_rotation_vector

    v = rng.normal(0, 1.0 if big else 0.03, 3)
    return np.asarray(as_rotation_matrix(from_rotation_vector(v)), float)


def rand_spec(rng):
    """(spec, index of the chain's only rotate stage or None)"""
    r = rng.random()
    enc = ("equirect_enc", bool(rng.random() < 0.85)) if r < 0.7 else ("fisheye_enc", MODELS[int(rng.integers(5))])
    mid = []
    n_rot = 0
    for _ in range(int(rng.choice([0, 0, 1, 1, 2, 3]))):
        k = rng.random()
        if k < 0.35:
            mid.append(("rot", rand_rot(rng, rng.random() < 0.4).tolist()))
            n_rot += 1
        elif k < 0.45:
            q = rng.normal(0, 1, 4)
            q[0] = abs(q[0]) + 0.5  # non-unit on purpose (cli.py:308-319 builds such quaternions)
            mid.append(("rot_quat", tuple(float(x) for x in q)))
            n_rot += 1
        elif k < 0.7:
            n = int(rng.integers(2, 6))
            co = [0.0, 1.0] + [float(x) for x in rng.normal(0, 0.08, n - 2)]
            if rng.random() < 0.3:
                co[0] = float(rng.normal(0, 0.02))
            mid.append(("poly", co))
        elif k < 0.9:
            mid.append(("zoom", float(rng.uniform(0.4, 2.5))))
        else:
            mid.append(("inverse", ("zoom", float(rng.uniform(0.5, 2.0)))))
    d = rng.random()
    if d < 0.75:
        dec = ("fisheye_dec", "equidistant")
    elif d < 0.93:
        dec = ("fisheye_dec", MODELS[int(rng.integers(5))])
    else:
        dec = ("rectilinear_dec", float(rng.uniform(8, 30)), float(rng.uniform(10, 40)))
    spec = [enc] + mid + [dec]
    rot_at = None
    if n_rot == 1:
        rot_at = [i for i, it in enumerate(spec) if it[0] in ("rot", "rot_quat")][0]
    return spec, rot_at


def rand_size(rng, big: float, lo: int = 1):
    r = rng.random()
    if r < big:
        return int(rng.integers(1200, 2700))
    if r < big + 0.35:
        return int(rng.integers(300, 1200))
    return int(rng.integers(lo, 300))


WIDE_BVS = [70000, -3, 2.5, 1.5, 0.25, (70000, -3, 2.5), (1.5, 0.25, -3, 2.5), (1e-40, 3e38, -1, 2), 0, 300, (12, 40000, 7.5, 65535)]
EXTREME_PIXELS = np.array([1e-45, -1e-45, 1e-39, 1.1754943508222875e-38, 3.4e38, -3.4e38, 0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)


def rand_pixels(rng, shape, dtype, extremes: bool = False) -> np.ndarray:
    """random pixels of a wide type: uint16 full scale; float32 around 120 with negatives, now and then (`extremes`) sprinkled with
    denormals, values next to FLT_MAX, signed zeros, infinities and NaN"""
    if dtype == np.uint16:
        return rng.integers(0, 65536, shape).astype(np.uint16)
    a = rng.normal(120.0, 90.0, shape).astype(np.float32)
    if extremes:
        m = rng.random(shape) < 0.05
        a[m] = rng.choice(EXTREME_PIXELS, int(m.sum()))
    return a


def neq(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """elementwise "differs": bytes for the integer types; float32: equal, with NaN <=> NaN"""
    if got.dtype != np.float32:
        return got != want
    return ~((got == want) | (np.isnan(got) & np.isnan(want)))


def make_view(rng, arr: np.ndarray, dev, allow_unaligned: bool):
    """the array as a device tensor: contiguous, or a column slice of a wider buffer (pitched; offset dword-aligned or not)"""
    h, w, cn = arr.shape
    if rng.random() < 0.5:
        return torch.from_numpy(arr).to(dev)
    pad_l = int(rng.integers(0, 9)) if allow_unaligned and rng.random() < 0.3 else 4 * int(rng.integers(0, 5))
    pad_r = int(rng.integers(0, 9)) if allow_unaligned and rng.random() < 0.3 else 4 * int(rng.integers(0, 5))
    if arr.dtype == np.uint8:
        wide = rng.integers(0, 256, (h, pad_l + w + pad_r, cn), dtype=np.uint8)
    else:  # (pads in pixels: an odd one leaves a uint16 view of cn 1 / 3 2-byte aligned only)
        wide = rand_pixels(rng, (h, pad_l + w + pad_r, cn), arr.dtype.type)
    wide[:, pad_l:pad_l + w] = arr
    return torch.from_numpy(wide).to(dev)[:, pad_l:pad_l + w]


DUMP = [False]
HOT = [0.3]  # share of the chain cases drawn from the shapes the tuned kernels serve (--hot)
GEN2 = [0.0]  # share of the chain cases forced into general mode 2 (--gen2)
KINDS: dict = {}  # kernel family -> launch groups it served (remapper.last_launch_kinds): which kernels the run reached
SINGULAR = [0]  # differing pixels among the ill-conditioned ones that are left out (module docstring)
TIES = [0]  # ... among those at a float32 rounding tie (float32_ties)
XF = {"drawn": 0, "refused": 0}  # compositions of the --jpegxf share, and those of them the restatement refuses
LAST_MASKED = [0.0]  # share of the last chain case's pixels that its masks left out (the largest over its units)
WIDE_CHAIN = {"run": 0, "not counted": 0, "masked px": 0, "px": 0}  # chain cases of --wide: a case with more than 5 % masked is not counted


def dump_diff(k, got, want, maps, pmaps=None, fill=None) -> None:
    """where unit k differs: counts, bounding box, the first pixels with their map coordinates (the oracle's and the product's)"""
    d = np.argwhere(neq(got, want).any(axis=2))
    print(f"  unit {k}: {len(d)} pixels differ, rows {d[:, 0].min()}..{d[:, 0].max()}, cols {d[:, 1].min()}..{d[:, 1].max()}; "
          f"rows mod 16 {sorted(set((d[:, 0] % 16).tolist()))[:16]}, cols//4 mod 16 {sorted(set(((d[:, 1] // 4) % 16).tolist()))[:16]}")
    for (j, i) in d[:12]:
        pm = "" if pmaps is None else f" product map=({pmaps[0][j, i]!r}, {pmaps[1][j, i]!r})"
        fl = "" if fill is None else f" prefill={fill[j, i].tolist()}"
        print(f"    (row {j}, col {i}) map=({maps[0][j, i]!r}, {maps[1][j, i]!r}){pm} got={got[j, i].tolist()} want={want[j, i].tolist()}{fl}")


def ill_conditioned(spec, radius, size_in, size_out) -> np.ndarray:
    """Pixels where the chain amplifies a perturbation of the output position by 1e6 or more (the fp64 map at positions shifted by
    1e-7 px against the map itself): the last bits of every intermediate -- which differ between libms and with fused multiply-adds
    -- decide the 1/32-pixel bucket there.  Poles of a projection, and stacked polynomial stages that take an angle to 1e12 rad."""
    W, H = size_out
    ch = O.chain_from_spec(spec, radius=radius, size_input=size_in, size_output=size_out)
    x0, y0 = O.get_map(ch, radius=radius, size_input=size_in, size_output=size_out, f64=True)
    ch.ops[0].p[0] -= 1e-7  # Normalize's centre: the same as every pixel 1e-7 further right / down
    ch.ops[0].p[1] -= 1e-7
    x1, y1 = O.get_map(ch, radius=radius, size_input=size_in, size_output=size_out, f64=True)
    with np.errstate(invalid="ignore", over="ignore"):
        amp = np.maximum(np.abs(x1 - x0), np.abs(y1 - y0)) / 1e-7
    return ~(amp < 1e6)



def float32_ties(spec, radius, size_in, size_out) -> np.ndarray:
    """Pixels whose float64 coordinate is a tie of the float64 -> float32 rounding to within 1e-14 (relative): the oracle's libm and the
    product's tables are each a few float64 ulps off the exact value, so the cast may go either way and the 1/32-pixel bucket with it.
    Measure zero; tools/fuzz_cpu.py met one such pixel (and its three mirror images) in 30 000 chains.  Only evaluated for a unit that
    still differs behind the ill-conditioned mask."""
    ch = O.chain_from_spec(spec, radius=radius, size_input=size_in, size_output=size_out)
    fx, fy = O.get_map(ch, radius=radius, size_input=size_in, size_output=size_out, f64=True)
    tie = np.zeros(fx.shape, bool)
    for v in (fx, fy):
        f = v.astype(np.float32)
        up, dn = np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))
        with np.errstate(invalid="ignore", over="ignore"):
            m1, m2 = (f.astype(np.float64) + up.astype(np.float64)) / 2, (f.astype(np.float64) + dn.astype(np.float64)) / 2
            tie |= np.minimum(np.abs(v - m1), np.abs(v - m2)) <= 1e-14 * np.abs(v)
    return tie

def one_case(rng, dev, big: float, dtype=np.uint8) -> tuple[str, int]:
    """runs one random case; returns (description, number of differing bytes).  `dtype` uint16 / float32 (--wide): the same chains, views,
    batches, pairs and masks with 16-bit or float32 pixels, against wide_ref.remap on the oracle's map, at sizes that keep the NumPy
    restatement in seconds"""
    wide = dtype != np.uint8
    LAST_MASKED[0] = 0.0
    spec, rot_at = rand_spec(rng)
    cn = int(rng.choice([3, 3, 3, 1, 4]))
    interp = int(rng.choice([1, 1, 1, 0, 2, 4, 4]))
    border = int(rng.choice([0, 0, 0, 0, 1, 2, 3, 4, 5]))
    bval = tuple(int(x) for x in rng.integers(0, 256, int(rng.integers(1, 5)))) if rng.random() < 0.7 else int(rng.integers(0, 256))
    pair = rng.random() < 0.3
    wo, ho = rand_size(rng, big), rand_size(rng, big)
    if rng.random() < 0.3:
        ho = wo
    ws, hs = rand_size(rng, big, 1), rand_size(rng, big, 1)
    if rng.random() < 0.4:
        ws = hs = max(ws, 1)
    if interp in (2, 4) and max(wo * ho, ws * hs) > 1500 * 1500:  # keep the oracle's K x K loops in seconds
        wo, ho = min(wo, 1400), min(ho, 1400)
    rsel = rng.random()
    radius = min(ws, hs) / 2 if rsel < 0.5 else float(rng.uniform(0.2, 1.6) * min(ws, hs) / 2) if rsel < 0.92 else -float(rng.uniform(5, 100))
    radius = float(max(radius, 1.0)) if radius > 0 else radius
    if pair:
        n = 2
    else:
        n = int(rng.choice([1, 1, 2, 3, 5, 8, 17, 33]))
        if wo * ho * n > 6e6:
            n = max(1, int(6e6 // (wo * ho)))
    use_rot = (rot_at is not None) and (not pair) and rng.random() < 0.5
    unaligned_views = True
    if rng.random() < HOT[0]:
        # the shapes the tuned kernels are selected for (the free grammar above reaches them once in a hundred cases): an unrotated
        # equirectangular -> equidistant chain (now and then with one polynomial, a zoom, or a rotate stage whose matrix the units
        # override), rays that stay in the front hemisphere (output about square, rows pairing up about the equator), outputs of 416
        # px and more (one table entry per lane), mostly bilinear + BORDER_CONSTANT, pairs / single images / batches / per-unit rotations
        mid = []
        rot_units = rng.random() < 0.3
        if rot_units:
            mid.append(("rot", np.eye(3).tolist()))
        pk = rng.random()
        if pk < 0.25:
            mid.append(("poly", [0.0, 1.0, float(rng.uniform(-0.15, 0.08))]))
        elif pk < 0.35:
            mid.append(("zoom", float(rng.uniform(0.8, 1.3))))
        spec = [("equirect_enc", True)] + mid + [("fisheye_dec", "equidistant")]
        rot_at = 1 if rot_units else None
        if (not rot_units) and rng.random() < 0.4:
            # round 5: the chains that left the interpreter -- planar (fisheye -> fisheye: the reference's own test chains,
            # tests/test_remapper.py:42-91), is_latitude_y=False, a rotation behind radial stages (baked into the plan)
            fam = rng.random()
            enc = ("equirect_enc", False) if fam < 0.25 else ("fisheye_enc", MODELS[int(rng.integers(5))])
            mid2 = list(mid)
            if rng.random() < 0.35:
                mid2.insert(int(rng.integers(0, len(mid2) + 1)), ("rot", rand_rot(rng, rng.random() < 0.5).tolist()))
            if fam >= 0.25 and rng.random() < 0.15:
                enc = ("equirect_enc", True)  # (equirect, radial stage, rotation: the S / Cm tables behind an EquirectangularEncoder)
                mid2 = [("poly", [0.0, 1.0, float(rng.uniform(-0.1, 0.05))]), ("rot", rand_rot(rng, False).tolist())]
            dec = ("fisheye_dec", "equidistant") if rng.random() < 0.7 else ("fisheye_dec", MODELS[int(rng.integers(5))])
            spec = [enc] + mid2 + [dec]
        cn = int(rng.choice([3, 3, 3, 3, 1, 4]))
        interp = int(rng.choice([1, 1, 1, 1, 1, 0, 2, 4]))
        border = int(rng.choice([0, 0, 0, 0, 0, 1, 4, 5]))
        ho = int(rng.integers(13, 66)) * 32 if rng.random() < 0.85 else int(rng.integers(416, 2100))
        if rng.random() < 0.15:
            ho = int(rng.integers(64, 417))  # small outputs (the reference's tests: 256 x 256): per-pixel table entries, tiny grids
        wo = max(1, ho + int(rng.choice([0, 0, 0, -64, -4, 4, 60, 64])) + (0 if rng.random() < 0.7 else int(rng.integers(-100, 30))))
        if interp in (2, 4):
            wo, ho = min(wo, 1100), min(ho, 1088)
        hs = int(rng.integers(60, 2600))
        ws = hs + (0 if rng.random() < 0.5 else int(rng.integers(-hs // 3, hs // 2)))
        if rng.random() < 0.7:
            ws = (ws + 3) & ~3  # (a width whose rows stay dword-aligned: the LDS-DMA kernels)
        radius = float(rng.uniform(0.3, 0.62) * min(ws, hs))
        shape = rng.random()
        pair = (not rot_units) and shape < 0.4
        n = 2 if pair else (1 if shape < 0.55 else int(rng.choice([2, 3, 4, 5, 8, 16, 17, 40])))
        if not pair and wo * ho * n > 2.5e7:
            n = max(1, int(2.5e7 // (wo * ho)))
        use_rot = rot_units
        unaligned_views = rng.random() < 0.15
    if GEN2[0] > 0 and rng.random() < GEN2[0]:  # (no draw when the option is off: earlier seeds replay as they ran)
        # general mode 2 on purpose (--gen2): radial stages / zooms IN FRONT of a rotation, so that the point enters 3-D through the S / Cm
        # tables -- with outputs far from square and zooms that push the base variable out of those tables for part of the image (lanes
        # whose pixels are split between the tile kernel and the fix-up pass: case 1974 of seed 34 was such a lane)
        enc = ("equirect_enc", bool(rng.random() < 0.8)) if rng.random() < 0.7 else ("fisheye_enc", MODELS[int(rng.integers(5))])
        pre = []
        for _ in range(int(rng.choice([1, 1, 2]))):
            k = rng.random()
            if k < 0.5:
                pre.append(("zoom", float(rng.uniform(0.5, 2.6))))
            elif k < 0.8:
                pre.append(("poly", [0.0, 1.0, float(rng.uniform(-0.2, 0.2))]))
            else:
                pre.append(("inverse", ("zoom", float(rng.uniform(0.5, 2.0)))))
        rots = [("rot", rand_rot(rng, rng.random() < 0.5).tolist()) for _ in range(int(rng.choice([1, 1, 2])))]
        post = [("poly", [0.0, 1.0, float(rng.uniform(-0.12, 0.06))])] if rng.random() < 0.3 else []
        dec = ("fisheye_dec", "equidistant") if rng.random() < 0.7 else ("fisheye_dec", MODELS[int(rng.integers(5))])
        spec = [enc] + pre + rots + post + [dec]
        rot_at, use_rot = None, False
        cn = int(rng.choice([3, 3, 3, 1, 4]))
        interp = int(rng.choice([1, 1, 1, 0, 2, 4]))
        border = int(rng.choice([0, 0, 0, 1, 4, 5]))
        wo, ho = int(rng.integers(64, 1300)), int(rng.integers(64, 1500))
        if interp in (2, 4):
            wo, ho = min(wo, 1000), min(ho, 1000)
        hs = int(rng.integers(60, 1200))
        ws = hs + (0 if rng.random() < 0.5 else int(rng.integers(-hs // 3, hs // 2)))
        radius = float(rng.uniform(0.3, 0.7) * min(ws, hs))
        pair = rng.random() < 0.4
        n = 2 if pair else int(rng.choice([1, 1, 2, 3]))
        unaligned_views = rng.random() < 0.15
    if wide:
        cap = 320 if interp in (2, 4) else 640
        wo, ho, ws, hs = min(wo, cap), min(ho, cap), min(ws, 1000), min(hs, 1000)
        if not pair and wo * ho * n > 3e5:
            n = max(1, int(3e5 // (wo * ho)))
        bval = WIDE_BVS[int(rng.integers(len(WIDE_BVS)))]
    rots = [rand_rot(rng, False) for _ in range(n)] if use_rot else None
    # units of different source sizes behind one transformer: the map is for images[0] (remapper.py:385), every image is
    # sampled within its own bounds; a pair of per-eye transformers (remapper.py:460-473): every eye its own chain and geometry
    mixed = (not pair) and (not use_rot) and n > 1 and rng.random() < 0.2
    tuple_t = pair and rng.random() < 0.25
    sizes = [(hs, ws)] * n
    if mixed or (tuple_t and rng.random() < 0.5):
        sizes = [(hs, ws)] + [(max(1, hs + int(rng.integers(-40, 41))), max(1, ws + int(rng.integers(-40, 41)))) for _ in range(n - 1)]
    spec2 = rand_spec(rng)[0] if tuple_t else None
    if wide:
        ext = rng.random() < 0.33
        imgs = [rand_pixels(rng, (h_, w_, cn), dtype, ext) for (h_, w_) in sizes]
    else:
        imgs = [rng.integers(0, 256, (h_, w_, cn), dtype=np.uint8) for (h_, w_) in sizes]
    if rng.random() < 0.3:  # a fisheye disc with a black surround, like the real inputs
        for im in imgs:
            yy, xx = np.mgrid[:im.shape[0], :im.shape[1]]
            im[((xx - im.shape[1] // 2) ** 2 + (yy - im.shape[0] // 2) ** 2) > (min(im.shape[:2]) / 2) ** 2] = 0
    fill = rand_pixels(rng, (ho, wo, cn), dtype) if wide else rng.integers(0, 256, (ho, wo, cn), dtype=np.uint8)
    desc = (f"{np.dtype(dtype).name} " if wide else "") + (f"spec={spec!r} cn={cn} interp={interp} border={border} bval={bval!r} out=({wo},{ho}) src=({ws},{hs}) radius={radius!r} n={n} pair={pair} "
            f"rots={use_rot}" + (f" sizes={sizes!r}" if sizes[1:] != sizes[:-1] else "") + (f" right_eye_spec={spec2!r}" if tuple_t else ""))
    t = CS.to_product(spec)
    srcs = [make_view(rng, im, dev, allow_unaligned=unaligned_views) for im in imgs]
    if pair:
        sbs = torch.from_numpy(np.concatenate([fill, fill], axis=1)).to(dev)
        tt = (t, CS.to_product(spec2)) if tuple_t else t
        V.apply_lr_tensors(tt, srcs[0], srcs[1], out=sbs, size_output=(wo, ho), interpolation=interp, boarder_mode=border, boarder_value=bval,
                           radius=radius)
        got = [sbs[:, :wo].cpu().numpy(), sbs[:, wo:].cpu().numpy()]
    else:
        dsts = [make_view(rng, fill.copy(), dev, allow_unaligned=unaligned_views) for _ in range(n)]
        kw = {}
        if use_rot:
            kw["rotations"] = rots
        V.remap_tensors(t, srcs, dsts, radius=radius, interpolation=interp, boarder_mode=border, boarder_value=bval, **kw)
        from vr180_convert_amd import remapper as _rm

        if rng.random() < 0.12 and n <= 16 and len(_rm.last_launch_kinds()) == 1 and _rm.last_launch_kinds() != ["lut"]:
            # the same launch recorded into a graph and replayed on restored destinations (plan_run is launch-only; a recorded launch
            # with a fix-up pass neither waits for nor records the plan's flag event)
            torch.cuda.synchronize()
            for d in dsts:
                d.copy_(torch.from_numpy(fill).to(dev))
            st = torch.cuda.Stream(device=dev)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=st):
                V.remap_tensors(t, srcs, dsts, radius=radius, interpolation=interp, boarder_mode=border, boarder_value=bval, **kw)
            for d in dsts:
                d.copy_(torch.from_numpy(fill).to(dev))
            torch.cuda.synchronize()
            gr.replay()
            torch.cuda.synchronize()
            desc += " graph-replayed"
        got = [d.cpu().numpy() for d in dsts]
    from vr180_convert_amd import remapper

    for kind in remapper.last_launch_kinds():
        KINDS[kind] = KINDS.get(kind, 0) + 1
    bad = 0
    maps = None
    sing = None
    for k in range(n):
        if use_rot:
            sp = list(spec)
            sp[rot_at] = ("rot", rots[k].tolist())
            maps = O.get_map(sp, radius=radius, size_input=(hs, ws), size_output=(wo, ho))
        elif tuple_t:  # every eye: its own chain, its own source geometry
            maps = O.get_map(spec if k == 0 else spec2, radius=radius, size_input=sizes[k], size_output=(wo, ho))
            sing = None
        elif maps is None:
            maps = O.get_map(spec, radius=radius, size_input=(hs, ws), size_output=(wo, ho))
        want = (W.remap if wide else O.remap)(imgs[k], maps[0], maps[1], interp, border, bval, dst=fill.copy())
        if use_rot or tuple_t or sing is None:
            sp_now = sp if use_rot else (spec2 if (tuple_t and k == 1) else spec)
            sing = ill_conditioned(sp_now, radius, sizes[k] if tuple_t else (hs, ws), (wo, ho))
            if border in (1, 2, 3, 4):
                sing |= ~((np.abs(maps[0]) < 2.0 ** 20) & (np.abs(maps[1]) < 2.0 ** 20))  # (NaN counts as singular)
        if sing is not None and sing.any():
            diff = neq(got[k], want).any(axis=2)
            SINGULAR[0] += int((diff & sing).sum())
            want = want.copy()
            want[sing] = got[k][sing]
            LAST_MASKED[0] = max(LAST_MASKED[0], float(sing.mean()))
            if wide:
                WIDE_CHAIN["masked px"] += int(sing.sum())
        if wide:
            WIDE_CHAIN["px"] += wo * ho
        if neq(got[k], want).any() and not use_rot:
            tie = float32_ties(spec2 if (tuple_t and k == 1) else spec, radius, sizes[k] if tuple_t else (hs, ws), (wo, ho))
            if tie.any():
                TIES[0] += int((neq(got[k], want).any(axis=2) & tie).sum())
                want = want.copy()
                want[tie] = got[k][tie]
        bad += int(neq(got[k], want).sum())
        if DUMP[0] and neq(got[k], want).any():
            pm = None
            try:
                sp_k = (spec2 if (tuple_t and k == 1) else spec) if not use_rot else sp
                pm = V.get_map(CS.to_product(sp_k), radius=radius, size_input=sizes[k] if tuple_t else (hs, ws), size_output=(wo, ho))
            except Exception as e:  # noqa: BLE001
                print("  (product map unavailable:", e, ")")
            dump_diff(k, got[k], want, maps, pm, fill)
    return desc, bad


def lut_case(rng, dev, dtype=np.uint8) -> tuple[str, int]:
    """cv2.remap alone (v1c_remap_lut, what chains with user-defined stages use) on random float32 maps: smooth, noisy, and
    sprinkled with the values the fixed-point conversion treats specially.  `dtype` uint16 / float32 (--wide): v1c_remap_lut_ex
    against wide_ref.remap, nothing left out"""
    wide = dtype != np.uint8
    import ctypes as C

    from vr180_convert_amd import _native
    from vr180_convert_amd.remapper import _stream_ptr, border_scalar

    cn = int(rng.choice([1, 3, 4]))
    interp = int(rng.choice([0, 1, 2, 3, 4]))
    border = int(rng.integers(0, 6))
    bval = tuple(int(x) for x in rng.integers(0, 256, int(rng.integers(1, 5))))
    hs, ws = int(rng.integers(1, 400)), int(rng.integers(1, 400))
    ho, wo = int(rng.integers(1, 500)), int(rng.integers(1, 500))
    if wide:
        if interp in (2, 4):
            ho, wo = min(ho, 300), min(wo, 300)
        bval = WIDE_BVS[int(rng.integers(len(WIDE_BVS)))]
        src = rand_pixels(rng, (hs, ws, cn), dtype, rng.random() < 0.33)
    else:
        src = rng.integers(0, 256, (hs, ws, cn), dtype=np.uint8)
    jj, ii = np.mgrid[:ho, :wo].astype(np.float64)
    kind = int(rng.integers(0, 3))
    if kind == 0:  # affine + noise
        a = rng.normal(0, 1, 6)
        xm = a[0] * ii + a[1] * jj + rng.uniform(-ws, 2 * ws) + rng.normal(0, 0.3, (ho, wo))
        ym = a[2] * ii + a[3] * jj + rng.uniform(-hs, 2 * hs) + rng.normal(0, 0.3, (ho, wo))
    elif kind == 1:  # anywhere around the source
        xm = rng.uniform(-40, ws + 40, (ho, wo))
        ym = rng.uniform(-40, hs + 40, (ho, wo))
    else:  # on the 1/32 grid and half-way between its points (ties of cvRound)
        xm = rng.integers(-64, 32 * ws + 64, (ho, wo)) / 32.0 + rng.choice([0.0, 1 / 64, -1 / 64, 1e-7], (ho, wo))
        ym = rng.integers(-64, 32 * hs + 64, (ho, wo)) / 32.0 + rng.choice([0.0, 1 / 64, -1 / 64, 1e-7], (ho, wo))
    xm, ym = xm.astype(np.float32), ym.astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, -3e9, 2.0 ** 26, -(2.0 ** 26), 67108863.0, 32767.0, 32767.5, 32768.0, -32768.0,
                        -32768.5, -32769.0, -0.5, -1.0, 0.0, -0.0, ws - 1.0, ws - 0.5, float(ws), hs - 1.0, float(hs), 1e-30, -1e-30], np.float32)
    for m in (xm, ym):
        k = int(rng.integers(0, max(2, m.size // 20)))
        m.reshape(-1)[rng.integers(0, m.size, k)] = rng.choice(special, k)
    pad = int(rng.integers(0, 3)) * 4
    xw = np.zeros((ho, wo + pad), np.float32)
    yw = np.zeros((ho, wo + pad), np.float32)
    xw[:, :wo], yw[:, :wo] = xm, ym
    fill = rand_pixels(rng, (ho, wo, cn), dtype) if wide else rng.integers(0, 256, (ho, wo, cn), dtype=np.uint8)
    s_d = make_view(rng, src, dev, allow_unaligned=True)
    d_d = make_view(rng, fill.copy(), dev, allow_unaligned=True)
    x_d, y_d = torch.from_numpy(xw).to(dev), torch.from_numpy(yw).to(dev)
    if wide:
        from vr180_convert_amd.remapper import DEPTHS, border_scalar_f64

        bv, es = border_scalar_f64(bval), src.dtype.itemsize
        rc = _native.lib().v1c_remap_lut_ex(dev.index, _stream_ptr(dev), s_d.data_ptr(), hs, ws, (s_d.stride(0) if hs > 1 else ws * cn) * es, cn,
                                            DEPTHS[s_d.dtype], d_d.data_ptr(), ho, wo, (d_d.stride(0) if ho > 1 else wo * cn) * es, x_d.data_ptr(),
                                            y_d.data_ptr(), x_d.stride(0) * 4, interp, border, bv.ctypes.data)
        _native.check(rc, "v1c_remap_lut_ex")
        KINDS["lut_ex"] = KINDS.get("lut_ex", 0) + 1
    else:
        bv = border_scalar(bval)
        rc = _native.lib().v1c_remap_lut(dev.index, _stream_ptr(dev), s_d.data_ptr(), hs, ws, s_d.stride(0), cn, d_d.data_ptr(), ho, wo, d_d.stride(0),
                                         x_d.data_ptr(), y_d.data_ptr(), x_d.stride(0) * 4, interp, border, bv.ctypes.data)
        _native.check(rc, "v1c_remap_lut")
    got = d_d.cpu().numpy()
    want = (W.remap if wide else O.remap)(src, xm, ym, interp, border, bval, dst=fill.copy())
    bad = int(neq(got, want).sum())
    desc = (f"{np.dtype(dtype).name} " if wide else "") + f"LUT cn={cn} interp={interp} border={border} bval={bval!r} out=({wo},{ho}) src=({ws},{hs}) maps={kind} map_pad={pad}"
    if bad and DUMP[0]:
        dump_diff(0, got, want, (xm, ym))
    return desc, bad


def api_case(rng, dev) -> tuple[str, int]:
    """the reference's own entry points on host arrays: apply() (remapper.py:324-403: a list of images, 2-D grayscale among them,
    radius 'auto' / 'max' / a number, the host pipeline behind it) and apply_lr() on arrays (merge=False)"""
    spec, _ = rand_spec(rng)
    t = CS.to_product(spec)
    interp = int(rng.choice([1, 1, 0, 2, 4]))
    border = int(rng.choice([0, 0, 0, 1, 2, 3, 4]))
    bval = int(rng.integers(0, 256)) if rng.random() < 0.5 else tuple(int(x) for x in rng.integers(0, 256, 3))
    wo, ho = int(rng.integers(1, 700)), int(rng.integers(1, 700))
    hs, ws = int(rng.integers(8, 500)), int(rng.integers(8, 500))
    gray2d = rng.random() < 0.2
    cn = 1 if gray2d else int(rng.choice([3, 3, 1, 4]))
    n = int(rng.choice([1, 2, 3, 7, 12]))
    lr = rng.random() < 0.35

    def disc():
        im = rng.integers(40, 256, (hs, ws) if gray2d else (hs, ws, cn), dtype=np.uint8)
        yy, xx = np.mgrid[:hs, :ws]
        r = min(hs, ws) * float(rng.uniform(0.3, 0.49))
        im[((xx - ws // 2) ** 2 + (yy - hs // 2) ** 2) > r * r] = 0  # black surround: radius='auto' finds an edge
        return im

    rsel = rng.random()
    # (a 2-D image with radius='auto' raises IndexError in the reference -- get_radius indexes three axes, transformer.py:128-131 -- and here)
    radius = "auto" if rsel < 0.35 and not gray2d else "max" if rsel < 0.7 else float(rng.uniform(0.3, 1.2) * min(hs, ws) / 2)

    def masked_diff(g, w, r_used):
        """differing bytes outside the ill-conditioned pixels (module docstring)"""
        sing = ill_conditioned(spec, r_used, (hs, ws), (wo, ho))
        if border in (1, 2, 3, 4):
            xm, ym = O.get_map(spec, radius=r_used, size_input=(hs, ws), size_output=(wo, ho))
            sing |= ~((np.abs(xm) < 2.0 ** 20) & (np.abs(ym) < 2.0 ** 20))
        d = (g != w)
        d = d.any(axis=2) if d.ndim == 3 else d
        SINGULAR[0] += int((d & sing).sum())
        return int((g != w)[~sing].sum())

    desc = f"API {'apply_lr' if lr else 'apply'} spec={spec!r} cn={'2-D' if gray2d else cn} interp={interp} border={border} bval={bval!r} out=({wo},{ho}) src=({ws},{hs}) radius={radius!r} n={2 if lr else n}"
    if lr and not gray2d and cn == 3:
        import tempfile

        from vr180_convert_amd import _io

        left, right = disc(), disc()
        with tempfile.TemporaryDirectory() as td:  # apply_lr saves (a PNG here: lossless) and returns nothing, like the reference
            out_p = Path(td) / "sbs.png"
            V.apply_lr(t, left_path=left, right_path=right, out_path=out_p, size_output=(wo, ho), interpolation=interp, boarder_mode=border,
                       boarder_value=bval, radius=radius, device=dev)
            got = _io.imread(out_p)
        want = O.apply_lr(spec, left, right, size_output=(wo, ho), interpolation=interp, radius=radius, border_mode=border, border_value=bval)
        got = np.asarray(got)
        if got.shape != want.shape:
            return desc, want.size
        r_used = O.get_radius_smart(radius, [left, right])
        return desc, masked_diff(got[:, :wo], want[:, :wo], r_used) + masked_diff(got[:, wo:], want[:, wo:], r_used)
    if (not gray2d) and cn == 3 and rng.random() < 0.25:
        # remap_sharded: apply_lr over a batch of frames by worker threads (one per listed device -- the one card several times)
        frames = [(disc(), disc()) if rng.random() < 0.5 else np.concatenate([disc(), disc()], axis=1) for _ in range(n)]
        ndev = int(rng.choice([1, 2, 3, 5]))
        rad = radius if not isinstance(radius, str) or radius == "max" else float(min(hs, ws) * 0.45)
        got = V.remap_sharded(t, frames, size_output=(wo, ho), interpolation=interp, boarder_mode=border, boarder_value=bval, radius=rad,
                              devices=[dev.index] * ndev)
        bad = 0
        for f, g in zip(frames, got):
            l_, r_ = (f if isinstance(f, tuple) else (f[:, :ws], f[:, ws:]))
            r_used = O.get_radius_smart(rad, [l_, r_])
            want = O.apply_lr(spec, np.ascontiguousarray(l_), np.ascontiguousarray(r_), size_output=(wo, ho), interpolation=interp, radius=rad,
                              border_mode=border, border_value=bval)
            g = np.asarray(g)
            bad += (masked_diff(g[:, :wo], want[:, :wo], r_used) + masked_diff(g[:, wo:], want[:, wo:], r_used)) if g.shape == want.shape else want.size
        return desc.replace("API apply", f"API remap_sharded x{ndev}"), bad
    imgs = [disc() for _ in range(n)]
    got = V.apply(t, in_paths=imgs, size_output=(wo, ho), interpolation=interp, boarder_mode=border, boarder_value=bval, radius=radius, device=dev)
    want = O.apply(spec, [im[..., None] if gray2d else im for im in imgs], size_output=(wo, ho), interpolation=interp, border_mode=border,
                   border_value=bval, radius=radius)
    bad = 0
    r_used = O.get_radius_smart(radius, [im[..., None] if gray2d else im for im in imgs])
    for g, w in zip(got, want):
        g = np.asarray(g)
        bad += masked_diff(g.reshape(w.shape), w, r_used) if g.size == w.size else w.size
        if gray2d and g.ndim != 2:
            bad += 1  # a 2-D image comes back 2-D (cv2.remap keeps the rank)
    return desc, bad


def auto_case(rng, dev) -> tuple[str, int]:
    """radius='auto' with the radius never leaving the device (v1c_plan_run_auto; remapper.py:62-90 + :51-57): synthetic image
    circles of random radius and offset, square-ish outputs, every interpolation (INTER_AREA included) and border mode, one
    transformer or one per eye, eyes of one shape or the two halves of an odd-width side-by-side frame -- against the oracle's
    apply_lr(radius='auto'); where the device-resident form declines (fix-up pass needed) the exact one is compared."""
    from vr180_convert_amd import remapper

    mid = []
    if rng.random() < 0.3:
        mid.append(("poly", [0.0, 1.0, float(rng.uniform(-0.15, 0.08))]))
    if rng.random() < 0.3:
        mid.insert(0, ("rot", rand_rot(rng, False).tolist()))
    spec = [("equirect_enc", True)] + mid + [("fisheye_dec", "equidistant" if rng.random() < 0.8 else MODELS[int(rng.integers(5))])]
    cn = int(rng.choice([3, 3, 3, 1, 4]))
    interp = int(rng.choice([4, 4, 1, 1, 0, 2, 3]))
    border = int(rng.choice([0, 0, 0, 1, 2, 3, 4, 5]))
    bv = tuple(int(v) for v in rng.integers(0, 256, 4)) if rng.random() < 0.5 else 0
    hs, ws = int(rng.integers(64, 900)), int(rng.integers(64, 900))
    if rng.random() < 0.6:
        ws = (ws + 3) & ~3
    wo = int(rng.integers(64, 1100))
    ho = wo if rng.random() < 0.7 else max(16, wo + int(rng.integers(-80, 80)))
    tuple_t = rng.random() < 0.25

    def disc(w):
        im = rng.integers(30, 256, (hs, w, cn), dtype=np.uint8)
        yy, xx = np.mgrid[:hs, :w]
        r = min(hs, w) * float(rng.uniform(0.25, 0.52))
        cx, cy = w / 2 + float(rng.uniform(-4, 4)), hs / 2 + float(rng.uniform(-4, 4))
        im[((xx - cx) ** 2 + (yy - cy) ** 2) > r * r] = 0
        return im

    if rng.random() < 0.2:  # the two halves of an odd-width side-by-side frame: W // 2 and W - W // 2 columns of one tensor
        wsbs = 2 * ws + 1
        frame = np.concatenate([disc(wsbs // 2), disc(wsbs - wsbs // 2)], axis=1)
        a, b = frame[:, : wsbs // 2], frame[:, wsbs // 2 :]
        fd = torch.from_numpy(frame).to(dev)
        la, lb = fd[:, : wsbs // 2], fd[:, wsbs // 2 :]
    else:
        a, b = disc(ws), disc(ws)
        la, lb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    desc = (f"AUTO spec={spec!r} cn={cn} interp={interp} border={border} bv={bv} out=({wo},{ho}) src=({a.shape[1]}|{b.shape[1]},{hs}) "
            f"tuple={tuple_t}")
    try:
        ra, rb = O.get_radius(a), O.get_radius(b)
    except IndexError:
        return desc + " (no black border: skipped)", 0
    t = CS.to_product(spec)
    tt = (t, t) if tuple_t else t
    sbs = V.apply_lr_tensors(tt, la, lb, size_output=(wo, ho), interpolation=interp, boarder_mode=border, boarder_value=bv, radius="auto",
                             auto_radius_on_device=True)
    form = remapper.last_auto_radius_form()
    KINDS["auto:" + form] = KINDS.get("auto:" + form, 0) + 1
    got = sbs.cpu().numpy()
    bad = 0
    for k, (im, r_used) in enumerate(((a, ra if tuple_t else max(ra, rb)), (b, rb if tuple_t else max(ra, rb)))):
        # (one shared transformer: images[0]'s geometry for both eyes, remapper.py:385; per-eye transformers: each its own)
        size_in = (hs, int(im.shape[1])) if tuple_t else (hs, int(a.shape[1]))
        xm, ym = O.get_map(spec, radius=r_used, size_input=size_in, size_output=(wo, ho))
        want = O.remap(im, xm, ym, interp, border, bv)
        g = got[:, k * wo:(k + 1) * wo]
        sing = ill_conditioned(spec, r_used, size_in, (wo, ho))
        if border in (1, 2, 3, 4):
            sing |= ~((np.abs(xm) < 2.0 ** 20) & (np.abs(ym) < 2.0 ** 20))
        d = (g != want).any(axis=2)
        SINGULAR[0] += int((d & sing).sum())
        bad += int((g != want)[~sing].sum())
    return desc + f" form={form}", bad


def fused_case(rng, dev) -> tuple[str, int]:
    """v1c_remap_fused through raw ctypes (the one-shot export a foreign host binds: INTEGRATION.md): a lowered chain, pointers and
    pitches, nothing of the Python plan cache in between."""
    from vr180_convert_amd import _native
    from vr180_convert_amd.chain import lower_for_get_map
    from vr180_convert_amd.remapper import _stream_ptr, border_scalar

    spec, _ = rand_spec(rng)
    cn = int(rng.choice([3, 3, 1, 4]))
    interp = int(rng.choice([1, 1, 0, 2, 4]))
    border = int(rng.choice([0, 0, 0, 1, 2, 3, 4, 5]))
    bval = tuple(int(x) for x in rng.integers(0, 256, 3))
    wo, ho = rand_size(rng, 0.05), rand_size(rng, 0.05)
    hs, ws = rand_size(rng, 0.05, 2), rand_size(rng, 0.05, 2)
    if interp in (2, 4):
        wo, ho = min(wo, 900), min(ho, 900)
    radius = float(rng.uniform(0.3, 1.3) * min(ws, hs) / 2 + 1.0)
    src = rng.integers(0, 256, (hs, ws, cn), dtype=np.uint8)
    fill = rng.integers(0, 256, (ho, wo, cn), dtype=np.uint8)
    s_d = make_view(rng, src, dev, allow_unaligned=True)
    d_d = make_view(rng, fill.copy(), dev, allow_unaligned=True)
    chain = lower_for_get_map(CS.to_product(spec), radius=radius, size_input=(hs, ws), size_output=(wo, ho))
    bv = border_scalar(bval)
    import ctypes as C

    rc = _native.lib().v1c_remap_fused(dev.index, _stream_ptr(dev), s_d.data_ptr(), hs, ws, s_d.stride(0), cn, d_d.data_ptr(), ho, wo, d_d.stride(0),
                                       C.byref(chain), interp, border, bv.ctypes.data)
    _native.check(rc, "v1c_remap_fused")
    got = d_d.cpu().numpy()
    xm, ym = O.get_map(spec, radius=radius, size_input=(hs, ws), size_output=(wo, ho))
    want = O.remap(src, xm, ym, interp, border, bval, dst=fill.copy())
    sing = ill_conditioned(spec, radius, (hs, ws), (wo, ho))
    if border in (1, 2, 3, 4):
        sing |= ~((np.abs(xm) < 2.0 ** 20) & (np.abs(ym) < 2.0 ** 20))
    d = (got != want).any(axis=2)
    SINGULAR[0] += int((d & sing).sum())
    return f"FUSED spec={spec!r} cn={cn} interp={interp} border={border} bval={bval!r} out=({wo},{ho}) src=({ws},{hs}) radius={radius!r}", int((got != want)[~sing].sum())


def radius_case(rng, dev) -> tuple[str, int]:
    """get_radius (transformer.py:108-140) as the device kernel against the oracle: random images with black margins, noise around the
    threshold, every channel count, pitched views, images wider than high and the other way round, none / several rises and falls"""
    from vr180_convert_amd.remapper import _get_radius_any

    cn = int(rng.choice([1, 3, 4]))
    h, w = int(rng.integers(1, 700)), int(rng.integers(1, 700))
    thr = int(rng.choice([10, 10, 1, 25, 200, 0, 255]))
    img = rng.integers(0, 30 if rng.random() < 0.5 else 256, (h, w, cn), dtype=np.uint8)
    if rng.random() < 0.8:  # black margins of random widths (possibly none, possibly everything)
        a, b = sorted(int(v) for v in rng.integers(0, w + 1, 2))
        c, d = sorted(int(v) for v in rng.integers(0, h + 1, 2))
        img[:, :a] = 0
        img[:, b:] = 0
        img[:c] = 0
        img[d:] = 0
    t = make_view(rng, img, dev, allow_unaligned=True)
    try:
        want = ("value", O.get_radius(img, thr))
    except IndexError:
        want = ("IndexError", None)
    try:
        got = ("value", _get_radius_any(t, thr))
    except IndexError:
        got = ("IndexError", None)
    return f"RADIUS cn={cn} size=({w},{h}) threshold={thr} want={want} got={got}", 0 if got == want else 1


def png_case(rng, dev) -> tuple[str, int]:
    """the device PNG encoder (encode_png_tensor) against its NumPy restatement (png_ref.encode), the file byte for byte: a remap result
    as it lies on the device (one eye's half of a side-by-side tensor now and then), or a synthetic image of tests/png_cases.py's
    generators -- run planes, noise, Fibonacci frequencies, noise above runs; gray / BGR / BGRA, 8- and 16-bit -- with random
    parameters, in a random view; either filter, a random band height"""
    import png_cases as PC
    import png_ref as PR

    filt = "up" if rng.random() < 0.5 else "paeth"
    if rng.random() < 0.35:
        spec, _ = rand_spec(rng)
        dtype = np.uint8 if rng.random() < 0.7 else np.uint16
        cn = int(rng.choice([3, 3, 1, 4]))
        wo, ho, hs, ws = (int(v) for v in rng.integers(1, 600, 4))
        src = rng.integers(0, 256, (hs, ws, cn), dtype=np.uint8) if dtype == np.uint8 else rand_pixels(rng, (hs, ws, cn), dtype)
        radius = float(rng.uniform(0.3, 1.2) * min(ws, hs) / 2 + 1.0)
        s_d = torch.from_numpy(src).to(dev)
        if rng.random() < 0.5:
            sbs = V.apply_lr_tensors(CS.to_product(spec), s_d, s_d, size_output=(wo, ho), interpolation=int(rng.choice([0, 1, 4])), radius=radius)
            t = sbs[:, wo:] if rng.random() < 0.5 else sbs
        else:
            t = torch.zeros((ho, wo, cn), dtype=s_d.dtype, device=dev)
            V.remap_tensors(CS.to_product(spec), [s_d], [t], radius=radius, interpolation=int(rng.choice([0, 1, 4])))
        img = np.ascontiguousarray(t.cpu().numpy())
        rows = None if rng.random() < 0.3 else int(rng.integers(1, ho + 1))
        desc = f"remap result {np.dtype(dtype).name} {tuple(img.shape)} contiguous={t.is_contiguous()} spec={spec!r} src=({ws},{hs}) radius={radius!r}"
    else:
        desc, img, rows = PC.random_image(rng)
        t = make_view(rng, img, dev, allow_unaligned=True)
        desc += f" contiguous={t.is_contiguous()} byte offset={t.storage_offset() * img.dtype.itemsize}"
    from vr180_convert_amd import png_device

    h, w, cn = img.shape
    rows_used = png_device.default_band_rows(h, 1 + w * cn * img.dtype.itemsize) if rows is None else rows
    got = V.encode_png_tensor(t, filter=filt, band_rows=rows)
    want = PR.encode(img, filter=filt, band_rows=rows_used)
    KINDS["png"] = KINDS.get("png", 0) + 1
    bad = abs(len(got) - len(want)) + sum(a != b for a, b in zip(got, want)) if got != want else 0
    return f"PNG filter={filt} band_rows={rows!r} {desc}", bad


def jpeg_case(rng, dev) -> tuple[str, int]:
    """the device JPEG encoder (encode_jpeg_tensor) against its NumPy restatement (jpg_ref.encode), the file byte for byte: a remap
    result as it lies on the device (one eye's half of a side-by-side tensor now and then), or a random image -- smooth, noise, flat,
    hard edges, sparse coefficients; gray / BGR / BGRA -- in a random view; any quality, either subsampling, a random restart interval"""
    import jpg_cases as JC
    import jpg_ref as JR

    quality = int(rng.choice([1, 10, 49, 50, 75, 90, 95, 100])) if rng.random() < 0.7 else int(rng.integers(1, 101))
    sub = "420" if rng.random() < 0.6 else "444"
    if rng.random() < 0.3:
        spec, _ = rand_spec(rng)
        cn = int(rng.choice([3, 3, 1, 4]))
        wo, ho, hs, ws = (int(v) for v in rng.integers(1, 400, 4))
        src = rng.integers(0, 256, (hs, ws, cn), dtype=np.uint8)
        radius = float(rng.uniform(0.3, 1.2) * min(ws, hs) / 2 + 1.0)
        s_d = torch.from_numpy(src).to(dev)
        if rng.random() < 0.5:
            sbs = V.apply_lr_tensors(CS.to_product(spec), s_d, s_d, size_output=(wo, ho), interpolation=int(rng.choice([0, 1, 4])), radius=radius)
            t = sbs[:, wo:] if rng.random() < 0.5 else sbs
        else:
            t = torch.zeros((ho, wo, cn), dtype=s_d.dtype, device=dev)
            V.remap_tensors(CS.to_product(spec), [s_d], [t], radius=radius, interpolation=int(rng.choice([0, 1, 4])))
        img = np.ascontiguousarray(t.cpu().numpy())
        desc = f"remap result {tuple(img.shape)} contiguous={t.is_contiguous()} spec={spec!r} src=({ws},{hs}) radius={radius!r}"
    else:
        h, w = (int(v) for v in (rng.integers(1, 40, 2) if rng.random() < 0.4 else rng.integers(1, 300, 2)))
        cn = int(rng.choice([3, 3, 1, 4]))
        kind = str(rng.choice(["smooth", "noise", "flat", "edges", "mixed"]))
        seed = int(rng.integers(0, 1 << 30))
        if kind == "smooth":
            img = JC.smooth(h, w, cn, seed)
        elif kind == "noise":
            img = JC.noise(h, w, cn, seed)
        elif kind == "flat":
            img = np.full((h, w, cn), int(rng.integers(0, 256)), np.uint8)
        elif kind == "edges":
            img = (JC.noise((h + 7) // 8, (w + 7) // 8, cn, seed) > 127).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w] * 255
            img = np.roll(img, int(rng.integers(0, 8)), axis=1)
        else:
            img = np.where(JC.noise(h, w, 1, seed) > 200, JC.noise(h, w, cn, seed + 1), JC.smooth(h, w, cn, seed + 2))
        img = np.ascontiguousarray(img)
        t = make_view(rng, img, dev, allow_unaligned=True)
        desc = f"{kind} {tuple(img.shape)} seed={seed} contiguous={t.is_contiguous()} byte offset={t.storage_offset()}"
    h, w, cn = img.shape
    m = 16 if (cn != 1 and sub == "420") else 8
    nmcu = -(-h // m) * -(-w // m)
    r = rng.random()
    restart = None if r < 0.25 else 1 if r < 0.35 else nmcu if r < 0.45 else 65535 if r < 0.5 else int(rng.integers(1, nmcu + 2))
    got = V.encode_jpeg_tensor(t, quality=quality, subsampling=sub, restart_mcus=restart)
    want = JR.encode(img, quality, sub, restart)
    KINDS["jpeg"] = KINDS.get("jpeg", 0) + 1
    bad = abs(len(got) - len(want)) + sum(a != b for a, b in zip(got, want)) if got != want else 0
    return f"JPEG quality={quality} subsampling={sub} restart_mcus={restart!r} {desc}", bad


def jpegbatch_case(rng, dev) -> tuple[str, int]:
    """the batched device JPEG encoder (encode_jpeg_tensors) against the single calls (encode_jpeg_tensor) and the restatement
    (jpg_ref.encode), every file byte for byte: a list of 1 to 12 random images up to 96 x 96 -- smooth, noise, flat, hard edges,
    mixed; gray / BGR / BGRA -- in random views, each with its own quality, subsampling and restart interval; now and then under a
    workspace budget that cuts the list into chunks, or with one image several times"""
    import jpg_cases as JC
    import jpg_ref as JR

    n = int(rng.integers(1, 13))
    imgs, ts, quality, subs, restarts, kinds = [], [], [], [], [], []
    for _ in range(n):
        if imgs and rng.random() < 0.15:  # the image in front once more, with parameters of its own
            img, t, kind = imgs[-1], ts[-1], "again"
        else:
            h, w = (int(v) for v in (rng.integers(1, 25, 2) if rng.random() < 0.4 else rng.integers(1, 97, 2)))
            cn = int(rng.choice([3, 3, 1, 4]))
            kind = str(rng.choice(["smooth", "noise", "flat", "edges", "mixed"]))
            seed = int(rng.integers(0, 1 << 30))
            if kind == "smooth":
                img = JC.smooth(h, w, cn, seed)
            elif kind == "noise":
                img = JC.noise(h, w, cn, seed)
            elif kind == "flat":
                img = np.full((h, w, cn), int(rng.integers(0, 256)), np.uint8)
            elif kind == "edges":
                img = (JC.noise((h + 7) // 8, (w + 7) // 8, cn, seed) > 127).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w] * 255
            else:
                img = np.where(JC.noise(h, w, 1, seed) > 200, JC.noise(h, w, cn, seed + 1), JC.smooth(h, w, cn, seed + 2))
            img = np.ascontiguousarray(img)
            t = make_view(rng, img, dev, allow_unaligned=True)
        h, w, cn = img.shape
        sub = "420" if rng.random() < 0.6 else "444"
        m = 16 if (cn != 1 and sub == "420") else 8
        nmcu = -(-h // m) * -(-w // m)
        r = rng.random()
        imgs.append(img), ts.append(t), kinds.append(f"{kind}{tuple(img.shape)}")
        quality.append(int(rng.choice([1, 10, 49, 50, 75, 90, 95, 100])) if rng.random() < 0.7 else int(rng.integers(1, 101)))
        subs.append(sub)
        restarts.append(None if r < 0.25 else 1 if r < 0.35 else nmcu if r < 0.45 else 65535 if r < 0.5 else int(rng.integers(1, nmcu + 2)))
    budget = None if rng.random() < 0.6 else int(rng.integers(1, 400_000))
    got = V.encode_jpeg_tensors(ts, quality=quality, subsampling=subs, restart_mcus=restarts, workspace_budget=budget)
    chunks = V.last_encode_batch_report()["chunks"]
    bad = 0 if len(got) == n and (budget is not None or chunks == 1) else 1
    for img, t, q, sub, restart, g in zip(imgs, ts, quality, subs, restarts, got):
        for want in (JR.encode(img, q, sub, restart), V.encode_jpeg_tensor(t, quality=q, subsampling=sub, restart_mcus=restart)):
            bad += abs(len(g) - len(want)) + sum(a != b for a, b in zip(g, want)) if g != want else 0
    KINDS["jpegbatch"] = KINDS.get("jpegbatch", 0) + 1
    return f"JPEG batch n={n} budget={budget!r} chunks={chunks} quality={quality} subsampling={subs} restart_mcus={restarts!r} {' '.join(kinds)}", bad


def jpegopt_case(rng, dev) -> tuple[str, int]:
    """the optimised Huffman tables of the device JPEG encoder (optimize=True) against the restatement (jpg_opt_ref.encode) and, for a
    list, against the single calls, every file byte for byte: 1 to 8 random images up to 160 x 160 -- smooth, noise, flat, hard edges,
    mixed, flat with a noise patch; gray / BGR / BGRA -- in random views, each with its own quality, subsampling and restart interval
    and its own choice of optimised or standard tables; now and then under a workspace budget that cuts the list into chunks.  Every
    optimised file must decode (Pillow) to the pixels of its standard-table file and not be larger than it by more than nothing: the
    scan may tie for a tiny image, the DHT segment always shrinks."""
    import jpg_cases as JC
    import jpg_opt_ref as JO
    import jpg_ref as JR

    n = int(rng.integers(1, 9))
    imgs, ts, quality, subs, restarts, opts, kinds = [], [], [], [], [], [], []
    for _ in range(n):
        h, w = (int(v) for v in (rng.integers(1, 25, 2) if rng.random() < 0.4 else rng.integers(1, 161, 2)))
        cn = int(rng.choice([3, 3, 1, 4]))
        kind = str(rng.choice(["smooth", "noise", "flat", "edges", "mixed", "patch"]))
        seed = int(rng.integers(0, 1 << 30))
        if kind == "smooth":
            img = JC.smooth(h, w, cn, seed)
        elif kind == "noise":
            img = JC.noise(h, w, cn, seed)
        elif kind == "flat":
            img = np.full((h, w, cn), int(rng.integers(0, 256)), np.uint8)
        elif kind == "edges":
            img = (JC.noise((h + 7) // 8, (w + 7) // 8, cn, seed) > 127).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w] * 255
        elif kind == "patch":
            img = np.full((h, w, cn), int(rng.integers(0, 256)), np.uint8)
            img[: (h + 3) // 4, : (w + 3) // 4] = JC.noise((h + 3) // 4, (w + 3) // 4, cn, seed)
        else:
            img = np.where(JC.noise(h, w, 1, seed) > 200, JC.noise(h, w, cn, seed + 1), JC.smooth(h, w, cn, seed + 2))
        img = np.ascontiguousarray(img)
        sub = "420" if rng.random() < 0.6 else "444"
        m = 16 if (cn != 1 and sub == "420") else 8
        nmcu = -(-h // m) * -(-w // m)
        r = rng.random()
        imgs.append(img), ts.append(make_view(rng, img, dev, allow_unaligned=True)), kinds.append(f"{kind}{tuple(img.shape)}")
        quality.append(int(rng.choice([1, 10, 49, 50, 75, 90, 95, 100])) if rng.random() < 0.7 else int(rng.integers(1, 101)))
        subs.append(sub)
        restarts.append(None if r < 0.25 else 1 if r < 0.35 else nmcu if r < 0.45 else 65535 if r < 0.5 else int(rng.integers(1, nmcu + 2)))
        opts.append(bool(rng.random() < 0.75))
    budget = None if rng.random() < 0.6 else int(rng.integers(1, 400_000))
    got = V.encode_jpeg_tensors(ts, quality=quality, subsampling=subs, restart_mcus=restarts, workspace_budget=budget, optimize=opts)
    chunks = V.last_encode_batch_report()["chunks"]
    bad = 0 if len(got) == n and (budget is not None or chunks == 1) else 1
    for img, t, q, sub, restart, o, g in zip(imgs, ts, quality, subs, restarts, opts, got):
        std = JR.encode(img, q, sub, restart)
        for want in (JO.encode(img, q, sub, restart, optimize=o), V.encode_jpeg_tensor(t, quality=q, subsampling=sub, restart_mcus=restart, optimize=o)):
            bad += abs(len(g) - len(want)) + sum(a != b for a, b in zip(g, want)) if g != want else 0
        if o and (len(g) >= len(std) or not np.array_equal(JR.decode(g), JR.decode(std))):
            bad += 1
    KINDS["jpegopt"] = KINDS.get("jpegopt", 0) + 1
    return (f"JPEG optimize n={n} budget={budget!r} chunks={chunks} optimize={opts} quality={quality} subsampling={subs} "
            f"restart_mcus={restarts!r} {' '.join(kinds)}"), bad


def jpegxc_case(rng, dev) -> tuple[str, int]:
    """the lossless JPEG transcoder (jpeg_transcode_device.transcode_regions) against its restatement (jpgxc_ref.transcode), the files
    byte for byte: a random image up to 160 x 160 -- smooth, noise, flat, mixed -- written by Pillow (grey, 4:4:4, 4:2:2 or 4:2:0, any quality,
    optimised tables now and then) or by the encoder's restatement (any restart interval), cut into one to three outputs of one to four
    random regions each -- crops, splits, swaps, shuffled strips --, each with its own restart interval (a row, none, any) and tables;
    now and then a list the contract refuses (overlapping or missing regions), which must be refused the restatement's way"""
    import jpg_cases as JC
    import jpg_ref as JR
    import jpgdec_cases as DC
    import jpgxc_ref as XR
    from vr180_convert_amd import jpeg_transcode_device as T

    h, w = (int(v) for v in rng.integers(1, 161, 2))
    quality = int(rng.choice([1, 10, 50, 75, 90, 95, 100])) if rng.random() < 0.7 else int(rng.integers(1, 101))
    kind = str(rng.choice(["smooth", "noise", "flat", "mixed"]))
    seed = int(rng.integers(0, 1 << 30))
    cn = 1 if rng.random() < 0.2 else 3
    if kind == "smooth":
        img = JC.smooth(h, w, cn, seed)
    elif kind == "noise":
        img = JC.noise(h, w, cn, seed)
    elif kind == "flat":
        img = np.full((h, w, cn), int(rng.integers(0, 256)), np.uint8)
    else:
        img = np.where(JC.noise(h, w, 1, seed) > 200, JC.noise(h, w, cn, seed + 1), JC.smooth(h, w, cn, seed + 2))
    img = np.ascontiguousarray(img)
    refuse = rng.random() < 0.08
    sampling = str(rng.choice(["420", "420", "444", "422"]))
    if sampling != "422" and rng.random() < 0.4:
        m = 16 if (cn != 1 and sampling == "420") else 8
        nmcu = -(-h // m) * -(-w // m)
        restart = 1 if rng.random() < 0.2 else int(rng.integers(1, nmcu + 2))
        data = JR.encode(img, quality, sampling, restart)
        how = f"jpg_ref restart_mcus={restart}"
    else:
        kw = {"optimize": True} if rng.random() < 0.3 else {}
        data = DC.pillow(img, quality, sampling, **kw)
        how = f"Pillow {kw!r}"
    mw = 8 if cn == 1 else {"444": 8, "422": 16, "420": 16}[sampling]
    mh = 16 if (cn == 3 and sampling == "420") else 8
    mcux, mcuy = -(-w // mw), -(-h // mh)
    outputs = []
    for _ in range(int(rng.integers(1, 4))):
        # strips of a random rectangle of the source, side by side in a random order (one strip: a crop; two: a swap)
        nx, ny = int(rng.integers(1, mcux + 1)), int(rng.integers(1, mcuy + 1))
        sx, sy = int(rng.integers(0, mcux - nx + 1)), int(rng.integers(0, mcuy - ny + 1))
        cuts = sorted(set([0, nx] + [int(v) for v in rng.integers(1, nx + 1, int(rng.integers(0, 4)))]))
        strips = [(a, b - a) for a, b in zip(cuts, cuts[1:])]
        order = rng.permutation(len(strips))
        regions, dx = [], 0
        for i in order:
            regions.append((sx + strips[i][0], sy, strips[i][1], ny, dx, 0))
            dx += strips[i][1]
        # the size: whole MCUs, or what the source shows of its last column and row, or any size inside the last MCUs
        ow = min(nx * mw, w - sx * mw) if rng.random() < 0.7 else nx * mw - int(rng.integers(0, mw))
        oh = min(ny * mh, h - sy * mh) if rng.random() < 0.7 else ny * mh - int(rng.integers(0, mh))
        r = rng.random()
        restart_out = None if r < 0.4 else 0 if r < 0.6 else 1 if r < 0.7 else int(rng.integers(1, nx * ny + 2))
        outputs.append(dict(width=ow, height=oh, regions=regions, restart_mcus=restart_out, optimize=bool(rng.random() < 0.3)))
    if refuse:
        o = outputs[int(rng.integers(0, len(outputs)))]
        if rng.random() < 0.5 or len(o["regions"]) == 1:
            o["regions"] = o["regions"] + [o["regions"][0]]        # the first region twice: an overlap
        else:
            o["regions"] = o["regions"][:-1]                       # a strip is missing: uncovered MCUs (or a region outside the output)
    KINDS["jpegxc"] = KINDS.get("jpegxc", 0) + 1
    desc = f"JPEGXC {kind} {(h, w, cn)} seed={seed} quality={quality} sampling={sampling} {how} outputs={outputs!r}"
    try:
        want = XR.transcode(data, outputs)
    except (XR.Unsupported, XR.Invalid) as e:
        kind_of = NotImplementedError if isinstance(e, XR.Unsupported) else ValueError
        try:
            T.transcode_regions(data, outputs, device=dev)
        except kind_of:
            return desc + f" refused ({type(e).__name__})", 0
        return desc + f" NOT refused ({type(e).__name__}: {e})", 1
    got = T.transcode_regions(data, outputs, device=dev)
    bad = sum(1 if len(a) != len(b) else int((np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8)).sum()) for a, b in zip(got, want))
    return desc, bad + abs(len(got) - len(want))


def jpegxf_draw(rng) -> tuple[list, list, str]:
    """a random composition: one to four files of one kind -- grey, 4:4:4, 4:2:2 or 4:2:0, up to 96 x 96, one quality (now and then one of
    them another), written by Pillow or by the encoder's restatement with any restart interval -- and one or two outputs, each a row of
    one to four strips, every strip a random rectangle of a random source under a random code, all of one height as they are placed;
    the strips of an output all transpose or none does (now and then they mix, which only symmetric tables allow); now and then a
    strip is doubled or dropped, which must be refused.  No device is touched: the draw is the same wherever it runs."""
    import jpg_cases as JC
    import jpg_ref as JR
    import jpgdec_cases as DC

    cn = 1 if rng.random() < 0.2 else 3
    sampling = str(rng.choice(["420", "420", "444", "422"]))
    mw = 8 if cn == 1 else {"444": 8, "422": 16, "420": 16}[sampling]
    mh = 16 if (cn == 3 and sampling == "420") else 8
    quality = int(rng.choice([50, 75, 90, 95, 100]))
    datas, grids, hows = [], [], []
    for _ in range(int(rng.integers(1, 5))):
        h, w = (int(v) for v in rng.integers(1, 97, 2))
        seed = int(rng.integers(0, 1 << 30))
        img = np.ascontiguousarray(JC.noise(h, w, cn, seed) if rng.random() < 0.3 else JC.smooth(h, w, cn, seed))
        q = quality if rng.random() < 0.96 else int(rng.integers(1, 101))
        if sampling != "422" and rng.random() < 0.4:
            restart = int(rng.integers(1, -(-h // mh) * -(-w // mw) + 2))
            datas.append(JR.encode(img, q, sampling, restart))
            hows.append(f"{(h, w)} seed={seed} q={q} jpg_ref restart_mcus={restart}")
        else:
            datas.append(DC.pillow(img, q, sampling))
            hows.append(f"{(h, w)} seed={seed} q={q} Pillow")
        grids.append((-(-w // mw), -(-h // mh)))
    square = mw == mh
    outputs = []
    for _ in range(int(rng.integers(1, 3))):
        transposing = square and rng.random() < 0.5
        mixed = square and rng.random() < 0.1
        H = int(rng.integers(1, min(min(g) for g in grids) + 1))
        regions, dx = [], 0
        for _ in range(int(rng.integers(1, 5))):
            si = int(rng.integers(0, len(datas)))
            t = bool(rng.integers(0, 2)) if mixed else transposing
            code = int(rng.integers(0, 4)) | (4 if t else 0)
            mcux, mcuy = grids[si]
            if t:
                nx, ny = H, int(rng.integers(1, mcuy + 1))
            else:
                nx, ny = int(rng.integers(1, mcux + 1)), H
            sx, sy = int(rng.integers(0, mcux - nx + 1)), int(rng.integers(0, mcuy - ny + 1))
            regions.append((si, code, sx, sy, nx, ny, dx, 0))
            dx += ny if t else nx
        ow = dx * mw - (0 if rng.random() < 0.6 else int(rng.integers(0, mw)))
        oh = H * mh - (0 if rng.random() < 0.6 else int(rng.integers(0, mh)))
        r = rng.random()
        restart_out = None if r < 0.4 else 0 if r < 0.6 else 1 if r < 0.7 else int(rng.integers(1, dx * H + 2))
        outputs.append(dict(width=ow, height=oh, regions=regions, restart_mcus=restart_out, optimize=bool(rng.random() < 0.3)))
    if rng.random() < 0.08:
        o = outputs[int(rng.integers(0, len(outputs)))]
        if rng.random() < 0.5 or len(o["regions"]) == 1:
            o["regions"] = o["regions"] + [o["regions"][0]]        # the first strip twice: an overlap
        else:
            o["regions"] = o["regions"][:-1]                       # the last strip is missing: uncovered MCUs
    return datas, outputs, f"JPEGXF cn={cn} sampling={sampling} sources=[{'; '.join(hows)}] outputs={outputs!r}"


def jpegxf_reference(datas, outputs):
    """(files, None) of the restatement (tests/jpgxf_ref.py), or (None, the exception it refuses the composition with)"""
    import jpgxf_ref as FR

    try:
        return FR.compose(datas, outputs), None
    except (FR.Unsupported, FR.Invalid) as e:
        return None, e


def jpegxf_case(rng, dev) -> tuple[str, int]:
    """the lossless JPEG composer (jpeg_compose_device.compose_regions) against its restatement (jpgxf_ref.compose), the files byte
    for byte; a composition the restatement refuses must be refused its way, which counts as agreement (the summary line says how many)"""
    import jpgxf_ref as FR
    from vr180_convert_amd import jpeg_compose_device as T

    datas, outputs, desc = jpegxf_draw(rng)
    named = [dict(o, regions=[(r[0], FR.NAMES[r[1]]) + tuple(r[2:]) for r in o["regions"]]) for o in outputs]
    KINDS["jpegxf"] = KINDS.get("jpegxf", 0) + 1
    XF["drawn"] += 1
    want, e = jpegxf_reference(datas, outputs)
    if e is not None:
        XF["refused"] += 1
        kind_of = NotImplementedError if isinstance(e, FR.Unsupported) else ValueError
        try:
            T.compose_regions(datas, named, device=dev)
        except kind_of:
            return desc + f" refused ({type(e).__name__})", 0
        return desc + f" NOT refused ({type(e).__name__}: {e})", 1
    got = T.compose_regions(datas, named, device=dev)
    bad = sum(1 if len(a) != len(b) else int((np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8)).sum()) for a, b in zip(got, want))
    return desc, bad + abs(len(got) - len(want))


def jpegdec_draw(rng) -> tuple[bytes, int, str]:
    """(file, components, description): a random image up to 96 x 96 -- smooth, noise, flat, mixed -- written by Pillow (grey, 4:4:4,
    4:2:2 or 4:2:0, any quality, optimised tables and its restart options now and then) or by the encoder's restatement (any restart
    interval)"""
    import jpg_cases as JC
    import jpg_ref as JR
    import jpgdec_cases as DC

    h, w = (int(v) for v in rng.integers(1, 97, 2))
    quality = int(rng.choice([1, 10, 50, 75, 90, 95, 100])) if rng.random() < 0.7 else int(rng.integers(1, 101))
    kind = str(rng.choice(["smooth", "noise", "flat", "mixed"]))
    seed = int(rng.integers(0, 1 << 30))
    cn = 1 if rng.random() < 0.2 else 3
    if kind == "smooth":
        img = JC.smooth(h, w, cn, seed)
    elif kind == "noise":
        img = JC.noise(h, w, cn, seed)
    elif kind == "flat":
        img = np.full((h, w, cn), int(rng.integers(0, 256)), np.uint8)
    else:
        img = np.where(JC.noise(h, w, 1, seed) > 200, JC.noise(h, w, cn, seed + 1), JC.smooth(h, w, cn, seed + 2))
    img = np.ascontiguousarray(img)
    if rng.random() < 0.3:
        sampling = "420" if rng.random() < 0.6 else "444"
        m = 16 if (cn != 1 and sampling == "420") else 8
        nmcu = -(-h // m) * -(-w // m)
        r = rng.random()
        restart = 1 if r < 0.2 else nmcu if r < 0.3 else 65535 if r < 0.4 else int(rng.integers(1, nmcu + 2))
        data = JR.encode(img, quality, sampling, restart)
        how = f"jpg_ref restart_mcus={restart}"
    else:
        sampling = str(rng.choice(["444", "422", "420"]))
        kw = {}
        if rng.random() < 0.3:
            kw["optimize"] = True
        r = rng.random()
        if r < 0.2:
            kw["restart_marker_blocks"] = int(rng.integers(1, 12))
        elif r < 0.35:
            kw["restart_marker_rows"] = int(rng.integers(1, 4))
        data = DC.pillow(img, quality, sampling, **kw)
        how = f"Pillow {kw!r}"
    return data, cn, f"{kind} {(h, w, cn)} seed={seed} quality={quality} sampling={sampling} {how}"


def jpegdec_case(rng, dev) -> tuple[str, int]:
    """the device JPEG decoder (decode_jpeg_tensor) against its restatement (jpgdec_ref.decode), the pixels byte for byte: a file of
    ``jpegdec_draw`` decoded at a random subsequence size"""
    import jpgdec_ref as DR

    data, cn, what = jpegdec_draw(rng)
    S = int(rng.choice([0, 256, 256, 288, 512, 1024, 4096]))
    channels = 1 if cn == 1 and rng.random() < 0.5 else 3
    got = V.decode_jpeg_tensor(data, channels=channels, subseq_bits=S or None).cpu().numpy()
    rep = V.last_decode_report()
    want = DR.decode(data, S, channels=channels, check=False)
    KINDS["jpegdec"] = KINDS.get("jpegdec", 0) + 1
    bad = int((got != want.pixels).sum()) if got.shape == want.pixels.shape else got.size
    bad += 0 if (rep["segments"], rep["subsequences"]) == (want.segments, want.subsequences) and rep["rounds"] <= want.rounds else 1
    return f"JPEGDEC {what} subseq_bits={S} channels={channels}", bad


def jpegprog_draw(rng) -> tuple[bytes, int, str]:
    """(file, components, description): a random image up to 64 x 64 written progressive by Pillow (its own script, restart options
    now and then), or its coefficients written again by jpgprog_cases.progressive with a random legal script -- DC interleaved, per
    component or in groups, random bands, point transforms up to 3 with their refinements in a random order, a restart interval of its
    own for any scan"""
    import jpg_cases as JC
    import jpgdec_cases as DC
    import jpgprog_cases as PC

    h, w = (int(v) for v in rng.integers(1, 65, 2))
    quality = int(rng.choice([10, 50, 75, 90, 95, 100]))
    kind = str(rng.choice(["smooth", "noise", "flat", "mixed"]))
    seed = int(rng.integers(0, 1 << 30))
    cn = 1 if rng.random() < 0.25 else 3
    if kind == "smooth":
        img = JC.smooth(h, w, cn, seed)
    elif kind == "noise":
        img = JC.noise(h, w, cn, seed)
    elif kind == "flat":
        img = np.full((h, w, cn), int(rng.integers(0, 256)), np.uint8)
    else:
        img = np.where(JC.noise(h, w, 1, seed) > 200, JC.noise(h, w, cn, seed + 1), JC.smooth(h, w, cn, seed + 2))
    img = np.ascontiguousarray(img)
    sampling = str(rng.choice(["444", "422", "420"]))
    if rng.random() < 0.35:
        kw = {}
        r = rng.random()
        if r < 0.25:
            kw["restart_marker_blocks"] = int(rng.integers(1, 12))
        elif r < 0.4:
            kw["restart_marker_rows"] = int(rng.integers(1, 4))
        data = DC.pillow(img, quality, sampling, progressive=True, **kw)
        how = f"Pillow {kw!r}"
    else:
        comps = list(range(cn))
        groups = [comps] if rng.random() < 0.5 else [[c] for c in comps] if rng.random() < 0.6 or cn == 1 else [[0], [1, 2]]
        chains = []
        for g in groups:                                   # DC: first scan and refinements of every group
            al = int(rng.integers(0, 3))
            chains.append([PC.scan(g, 0, 0, 0, al)] + [PC.scan(g, 0, 0, a, a - 1) for a in range(al, 0, -1)])
        dc = [sc for ch in chains for sc in ch[:1]]
        chains = [ch[1:] for ch in chains if len(ch) > 1]
        for c in comps:                                    # AC: random bands, each a chain of its own
            cuts = sorted(set(int(v) for v in rng.integers(2, 64, int(rng.integers(0, 4)))))
            for a, e in zip([1] + cuts, [v - 1 for v in cuts] + [63]):
                al = int(rng.integers(0, 4)) if rng.random() < 0.6 else 0
                chains.append([PC.scan([c], a, e, 0, al)] + [PC.scan([c], a, e, k, k - 1) for k in range(al, 0, -1)])
        script = dc
        while chains:                                      # the chains interleaved at random, each in its own order
            i = int(rng.integers(0, len(chains)))
            script.append(chains[i].pop(0))
            if not chains[i]:
                chains.pop(i)
        for sc in script:
            if rng.random() < 0.25:
                sc["dri"] = int(rng.choice([0, 1, 2, 3, 7, 65535]))
        data = PC.from_sequential(DC.pillow(img, quality, sampling), script)
        how = f"writer scans={len(script)} " + " ".join(f"{''.join(map(str, sc['comps']))}:{sc['Ss']}-{sc['Se']}:{sc['Ah']}{sc['Al']}" +
                                                           (f":dri{sc['dri']}" if sc["dri"] is not None else "") for sc in script)
    return data, cn, f"{kind} {(h, w, cn)} seed={seed} quality={quality} sampling={sampling} {how}"


def jpegprog_case(rng, dev) -> tuple[str, int]:
    """the device decoder of progressive JPEG files (decode_jpeg_tensor(progressive=True)) against its restatement
    (jpgprog_ref.decode): the pixels byte for byte, the rounds of every scan and the report, of a file of ``jpegprog_draw`` decoded
    at a random subsequence size"""
    import jpgprog_ref as PR

    data, cn, what = jpegprog_draw(rng)
    S = int(rng.choice([0, 256, 256, 288, 512, 1024]))
    channels = 1 if cn == 1 and rng.random() < 0.5 else 3
    got = V.decode_jpeg_tensor(data, channels=channels, subseq_bits=S or None, progressive=True).cpu().numpy()
    rep = V.last_decode_report()
    want = PR.decode(data, S, channels=channels, check=False)
    KINDS["jpegprog"] = KINDS.get("jpegprog", 0) + 1
    bad = int((got != want.pixels).sum()) if got.shape == want.pixels.shape else got.size
    bad += 0 if (rep["scans"], rep["segments"], rep["subsequences"], rep["scan_rounds"]) == (want.scans, want.segments, want.subsequences,
                                                                                             want.scan_rounds) else 1
    return f"JPEGPROG {what} subseq_bits={S} channels={channels}", bad


DMG = {"drawn": 0, "refused": 0, "decoded": 0, "parse": 0}  # jpegdmg cases by the restatement's verdict (parse: unsupported too)


def jpegdmg_draw(rng) -> tuple[str, bytes, bool, int]:
    """(description, file, whether it is progressive, subsequence size) of a --jpegdmg case: a file of ``jpegdec_draw`` or
    ``jpegprog_draw`` with one random damage of tests/jpgdmg_cases.py's kinds inside the entropy-coded bytes of one scan (a kind the
    file has no scan for -- two restart segments to exchange, a scan without markers to fill -- becomes a flipped bit)"""
    import jpgdmg_cases as M

    prog = bool(rng.random() < 0.4)
    data, cn, what = (jpegprog_draw if prog else jpegdec_draw)(rng)
    kind = str(rng.choice(M.RANDOM_KINDS))
    seed = int(rng.integers(0, 1 << 30))
    hurt = M.draw(data, prog, kind, np.random.default_rng(seed))
    if hurt is None:
        kind = "bitflip"
        hurt = M.draw(data, prog, kind, np.random.default_rng(seed))
    S = int(rng.choice([256, 256, 288, 512, 1024]))
    return f"JPEGDMG {'progressive' if prog else 'sequential'} {what} damage={kind} damage_seed={seed} subseq_bits={S}", hurt, prog, S


def jpegdmg_device(data, prog, S, h, w) -> tuple:
    """(code, error bit, error scan, rounds, pixels) of the device through the C ABI; h, w: the output to allocate"""
    import ctypes as C

    from vr180_convert_amd import _abi, _native
    from vr180_convert_amd.jpeg_decode_device import _Report

    lib = _native.lib()
    out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if prog:
        rep = _abi.JpegProgReport()
        rc = lib.v1c_jpeg_prog_decode(0, st, data, len(data), out.data_ptr(), 3 * w, 3, S, C.byref(rep), None, 0)
        return rc, int(rep.error_pos), int(rep.error_scan), int(rep.rounds), out.cpu().numpy()
    rep = _Report()
    rc = lib.v1c_jpeg_decode(0, st, data, len(data), out.data_ptr(), 3 * w, 3, S, C.byref(rep))
    return rc, int(rep.error_pos), 0, int(rep.rounds), out.cpu().numpy()


def jpegdmg_case(rng, dev) -> tuple[str, int]:
    """a damaged scan through the device decoders against the restatement's verdict (jpgdmg_cases.verdict_of): the code, the smallest
    bad bit and its scan, the rounds also of a refused file, and the pixels of damage that is still a legal stream"""
    import jpgdmg_cases as M

    desc, data, prog, S = jpegdmg_draw(rng)
    want = M.verdict_of(data, S, prog)
    DMG["drawn"] += 1
    DMG[want.what if want.what in ("refused", "decoded") else "parse"] += 1
    KINDS["jpegdmg"] = KINDS.get("jpegdmg", 0) + 1
    return jpegdmg_compare(desc, data, prog, S, want)


def jpegdmg_compare(desc, data, prog, S, want) -> tuple[str, int]:
    """the device decoder's answer for a file against a verdict of jpgdmg_cases.verdict_of"""
    import jpgdmg_cases as M

    h, w = want.pixels.shape[:2] if want.what == "decoded" else (8, 8)
    if want.what == "refused":
        s = (M.P.parse if prog else M.D.parse)(data)
        h, w = s.h, s.w
    rc, bit, scan, rounds, px = jpegdmg_device(data, prog, S, h, w)
    bad = 0 if rc == {"decoded": 0, "unsupported": -2, "parse": -5, "refused": -5}[want.what] else 1
    if want.what in ("decoded", "refused"):
        bad += 0 if rounds == want.rounds else 1
    if want.what == "refused":
        bad += 0 if (bit, scan) == (want.bit, want.scan) else 1
    if want.what == "decoded" and rc == 0:
        bad += int((px != want.pixels).sum())
    return f"{desc} restatement: {want.what} bit={want.bit} scan={want.scan} rounds={want.rounds}; device: rc={rc} bit={bit} scan={scan} rounds={rounds}", bad


ODD = {"drawn": 0, "legal": 0, "damage": 0, "refused": 0}  # jpegodd cases; refused: by the parse or the last pass, as the restatement predicts


def jpegodd_draw(rng) -> tuple[str, bytes, bool, int]:
    """(description, file, whether it is progressive, subsequence size) of a --jpegodd case: one legal file of unusual structure --
    drawn Huffman code shapes and table slots, quantisation slots and widths, component ids, segment orders, fill bytes, DRI oddities
    (tests/jpgodd_cases.py: random_legal, one file in four progressive) -- or one small supported file with one damage in a marker segment (random_damage)"""
    import jpgodd_cases as O

    if rng.random() < 0.5:
        desc, data, prog = O.random_legal(rng)
    else:
        desc, data, prog = O.random_damage(rng)
    S = int(rng.choice([256, 256, 288, 512, 1024]))
    return f"JPEGODD {'progressive' if prog else 'sequential'} {desc} subseq_bits={S}", data, prog, S


def jpegodd_case(rng, dev) -> tuple[str, int]:
    """an odd legal file or a damaged header through the device decoders against the restatement (jpgodd_cases.header_verdict_of):
    the parse's class and the byte it stops at, and for what the parse takes the code, the bad bit and its scan, the rounds and the pixels"""
    import jpgdmg_cases as M
    import jpgodd_cases as O

    desc, data, prog, S = jpegodd_draw(rng)
    v = O.header_verdict_of(data, S, prog)
    want = v.inner if v.inner is not None else M.Verdict("unsupported" if v.what == "unsupported" else "parse")
    ODD["drawn"] += 1
    ODD["legal" if " odd legal " in desc else "damage"] += 1
    ODD["refused"] += want.what != "decoded"
    KINDS["jpegodd"] = KINDS.get("jpegodd", 0) + 1
    if v.inner is not None:
        return jpegdmg_compare(desc, data, prog, S, want)
    # refused by the parse: the code, and the byte the parse stopped at in the report's error_pos
    rc, pos, _, _, _ = jpegdmg_device(data, prog, S, 8, 8)
    bad = (0 if rc == (-2 if v.what == "unsupported" else -5) else 1) + (0 if pos == v.pos else 1)
    return f"{desc} restatement's parse: {v.what} at byte {v.pos} ({v.why}); device entry: rc={rc} error_pos={pos}", bad


FEAT = {"drawn": 0, "refused": 0}  # feat cases drawn / of them refused by v1c_feat_detect as feat_ref.refusal predicts (not counted)
FEAT_IMAGES = ["disc", "noise", "low", "scene", "sphere", "flat"]
FEAT_RATIOS = [(3, 4), (1, 1), (1, 2), (0, 1)]


def circle_image(rng) -> tuple[np.ndarray, str]:
    """an (H, W, C) uint8 / uint16 frame: a disc (often clipped, sometimes with a dark wedge), speckle, hot pixels, or nothing"""
    import circle_cases as CC

    h, w = (int(rng.integers(1, 400)), int(rng.integers(1, 400))) if rng.random() < 0.85 else (int(rng.integers(400, 1600)), int(rng.integers(400, 1600)))
    cn = int(rng.choice([1, 3, 4]))
    dtype = np.uint16 if rng.random() < 0.3 else np.uint8
    kind = str(rng.choice(["disc", "disc", "clipped", "wedge", "speckle", "hot", "black", "lit"]))
    top = int(np.iinfo(dtype).max)
    cx, cy = w * rng.uniform(0.3, 0.7), h * rng.uniform(0.3, 0.7)
    r = min(h, w) * (rng.uniform(0.2, 0.45) if kind != "clipped" else rng.uniform(0.45, 0.8))
    a = CC.disc(h, w, cx, cy, r, cn=cn, dtype=dtype, value=int(rng.integers(top // 8, top + 1)), aa=bool(rng.random() < 0.7))
    if kind == "wedge":
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        a[y0:y0 + int(rng.integers(1, h // 3 + 2)), x0:x0 + int(rng.integers(1, w // 3 + 2))] = 0
    elif kind == "speckle":
        a[rng.random((h, w)) < rng.uniform(0.05, 0.6)] = top // 3
    elif kind == "hot":
        for _ in range(int(rng.integers(1, 60))):
            a[int(rng.integers(0, h)), int(rng.integers(0, w))] = top
    elif kind == "black":
        a[:] = 0
    elif kind == "lit":
        a[:] = top
    return a, f"{kind} {h}x{w}x{cn} {np.dtype(dtype).name} centre ({cx:.2f}, {cy:.2f}) r {r:.2f}"


def circle_case(rng, dev) -> tuple[str, int]:
    """v1c_fit_circle against tests/circle_ref.py; then, for 8-bit three-channel frames, a remap with random off-centre centres"""
    import circle_ref as CR
    from vr180_convert_amd import circle, remapper

    CIRCLE["drawn"] += 1
    if rng.random() < 0.3:
        return circle_remap_case(rng, dev)
    a, desc = circle_image(rng)
    h, w, cn = a.shape
    kw: dict = {}
    if rng.random() < 0.4:
        kw = dict(threshold=int(rng.choice([0, 1, 10, 40, 255, 65535])), run=int(rng.choice([1, 2, 4, 9, 64])),
                  min_points=int(rng.choice([3, 8, 50])), tol16=[int(v) for v in rng.integers(1, 300, int(rng.integers(0, 9)))])
    view = str(rng.choice(["contiguous", "pitched", "odd"]))
    if view == "contiguous":
        t = torch.from_numpy(a).to(dev)
    else:  # a slice of a wider (and, for "odd", one row and one column shifted) frame: pitched rows, an odd element offset
        pad = int(rng.integers(1, 40))
        base = np.zeros((h + 1, w + pad + 1, cn), a.dtype)
        oy, ox = (1, 1) if view == "odd" else (0, 0)
        base[oy:oy + h, ox:ox + w] = a
        t = torch.from_numpy(base).to(dev)[oy:oy + h, ox:ox + w]
    desc = f"circle {desc} view {view} {kw}"
    out, rim = circle.fit_circle_raw(t, points=True, **kw)
    wout, wrim = CR.fit(a, **kw)
    if rim.shape != wrim.shape:
        return desc + f" points {len(rim)} != {len(wrim)}", max(1, abs(len(rim) - len(wrim)))
    bad = int((rim != wrim).any(axis=1).sum()) + int((out[3:6] != wout[3:6]).sum())
    if not bad and np.abs(out - wout).max() > 1e-9:
        return desc + f" floats {out} != {wout}", 1
    return desc, bad


COLORMATCH = {"drawn": 0}


def colormatch_case(rng, dev) -> tuple[str, int]:
    """color_match_luts_tensor + apply_luts_tensor against tests/colormatch_ref.py, byte for byte: histograms, tables, report, the
    result and every byte of the buffer around the eyes"""
    import colormatch_cases as CC
    import colormatch_ref as CMR
    from vr180_convert_amd import colormatch

    COLORMATCH["drawn"] += 1
    h, w = (int(rng.integers(1, 200)), int(rng.integers(1, 300))) if rng.random() < 0.85 else (int(rng.integers(200, 900)), int(rng.integers(300, 1400)))
    cn = int(rng.choice([1, 3, 4]))
    kind = str(rng.choice(["noise", "flat", "gradient", "disc", "disc", "discs_apart", "black"]))
    seed = int(rng.integers(0, 1 << 30))
    if kind == "noise":
        L = np.random.default_rng(seed).integers(0, 256, (h, w, cn), dtype=np.uint8)
    elif kind == "flat":
        L = np.full((h, w, cn), int(rng.integers(0, 256)), np.uint8)
    elif kind == "gradient":
        L = np.broadcast_to((np.arange(w) * 255 // max(1, w - 1)).astype(np.uint8)[None, :, None], (h, w, cn)).copy()
    elif kind == "black":
        L = np.zeros((h, w, cn), np.uint8)
    else:
        L = CC.noise_disc(h, w, cn, seed, lo=int(rng.integers(0, 40)), hi=int(rng.integers(60, 256)), cx=w * rng.uniform(0.3, 0.7),
                          cy=h * rng.uniform(0.3, 0.7), r=min(h, w) * rng.uniform(0.2, 0.6))
    how = str(rng.choice(["brighter", "affine", "gamma", "same", "other"]))
    if how == "brighter":
        Rr = CC.brighter(L)
    elif how == "affine":
        Rr = np.clip(L.astype(np.int32) * int(rng.integers(2, 9)) // 4 + int(rng.integers(-30, 30)), 0, 255).astype(np.uint8)
    elif how == "gamma":
        Rr = (255.0 * (L / 255.0) ** rng.uniform(0.5, 2.0)).astype(np.uint8)
    elif how == "same":
        Rr = L.copy()
    else:
        Rr = np.random.default_rng(seed + 1).integers(0, 256, (h, w, cn), dtype=np.uint8)
    if kind == "discs_apart":  # the eyes' surrounds differ
        Rr = np.roll(Rr, (int(rng.integers(-h // 3 - 1, h // 3 + 1)), int(rng.integers(-w // 3 - 1, w // 3 + 1))), axis=(0, 1))
    kw: dict = dict(mode=str(rng.choice(["histogram", "gain"])), reference=str(rng.choice(["left", "right"])))
    if rng.random() < 0.5:
        lo = int(rng.integers(0, 120))
        kw.update(lo=lo, hi=int(rng.integers(lo, 256)), max_shift=int(rng.choice([0, 1, 20, 64, 255])), min_pixels=int(rng.choice([0, 1, 100, 1024])))
    layout = str(rng.choice(["separate", "padded", "sbs", "sbs_padded"]))
    lay = dict(off=int(rng.integers(0, 17)))
    if layout == "padded":
        lay.update(pad_l=int(rng.integers(0, 40)), pad_r=int(rng.integers(0, 40)))
    elif layout.startswith("sbs"):
        lay.update(sbs=True, pad=int(rng.integers(0, 40)) if layout == "sbs_padded" else 0)
    case = CC.carve(L, Rr, kw=kw, inplace=bool(rng.random() < 0.5), **lay)
    desc = f"colormatch {kind}/{how} {h}x{w}x{cn} {layout} {lay} inplace {case.inplace} {kw}"
    base_t = torch.from_numpy(case.base.copy()).to(dev)
    left, right = (torch.as_strided(base_t, (h, w, cn), (p_, cn, 1), off) for off, p_ in (case.left, case.right))
    ws = torch.full((2, 3, 256), -1, dtype=torch.int32, device=dev)
    luts, report = colormatch.color_match_luts_tensor(left, right, workspace=ws, **kw)
    tgt = right if case.target == "right" else left
    out = colormatch.apply_luts_tensor(tgt, luts, out=tgt if case.inplace else None)
    wres, wluts, wrep, whist = CC.reference_of(case)
    bad = int((ws.cpu().numpy().view(np.uint32) != whist).sum()) + int((luts.cpu().numpy() != wluts).sum()) + int((report.cpu().numpy() != wrep).sum())
    bad += int((out.cpu().numpy() != wres).sum()) + int((base_t.cpu().numpy() != CC.expected_base(case, wres)).sum())
    return desc, bad


VIGNETTE = {"drawn": 0}


def vignette_case(rng, dev) -> tuple[str, int]:
    """vignette_rings_tensor + apply_vignette_tensor against tests/vignette_ref.py, byte for byte: the ring record, the result and every
    byte of the buffer around the image"""
    import vignette_cases as VC
    from vr180_convert_amd import vignette as VG

    VIGNETTE["drawn"] += 1
    h, w = (int(rng.integers(1, 200)), int(rng.integers(1, 300))) if rng.random() < 0.85 else (int(rng.integers(200, 900)), int(rng.integers(300, 1400)))
    cn = int(rng.choice([1, 3, 4]))
    dtype = np.uint8 if rng.random() < 0.5 else np.uint16
    top = 255 if dtype == np.uint8 else 65535
    kind = str(rng.choice(["noise", "noise", "flat", "gradient", "black", "white"]))
    seed = int(rng.integers(0, 1 << 30))
    if kind == "noise":
        img = np.random.default_rng(seed).integers(0, top + 1, (h, w, cn)).astype(dtype)
    elif kind == "gradient":
        img = np.broadcast_to((np.arange(w) * top // max(1, w - 1)).astype(dtype)[None, :, None], (h, w, cn)).copy()
    else:
        img = np.full((h, w, cn), 0 if kind == "black" else top if kind == "white" else int(rng.integers(0, top + 1)), dtype)
    center = (int(rng.integers(-w, 2 * w)), int(rng.integers(-h, 2 * h))) if rng.random() < 0.3 else (int(rng.integers(0, w)), int(rng.integers(0, h)))
    radius = float(rng.choice([1.0, 2.0, 0.5 * max(h, w), 0.5 * min(h, w) + 0.5, rng.uniform(1.0, 3.0 * max(h, w))]))
    k = lambda: (float(rng.uniform(-0.6, 0.3)), float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.2, 0.2)))  # noqa: E731
    coefs = ((k(), k(), k()), float(rng.choice([1.0, 1.0, 2.2, rng.uniform(0.5, 3.0)])))
    if rng.random() < 0.1:
        coefs = VC.IDENTITY
    lo = int(rng.integers(0, top // 2))
    hi = int(rng.integers(lo, top + 1))
    if rng.random() < 0.5:
        lo, hi = VG.default_mask(dtype)
    es = np.dtype(dtype).itemsize
    lay = dict(off=es * int(rng.integers(0, 17)), pad=es * int(rng.integers(0, 40)) if rng.random() < 0.5 else 0, sbs=bool(rng.random() < 0.4))
    case = VC.carve(img, center=center, radius=radius, coefs=coefs, rings=int(rng.choice([16, 17, 64, 256, 1000, 1024])), lo=lo, hi=hi,
                    inplace=bool(rng.random() < 0.5), **lay)
    desc = (f"vignette {kind} {np.dtype(dtype).name} {h}x{w}x{cn} {lay} centre {center} radius {radius:.3f} rings {case.rings} mask [{lo}, {hi}] "
            f"inplace {case.inplace} {coefs}")
    base_t = torch.from_numpy(case.base.copy()).to(dev)
    typed = base_t if es == 1 else base_t[: base_t.numel() // 2 * 2].view(torch.uint16)
    image = torch.as_strided(typed, (h, w, cn), (case.pitch // es, cn, 1), case.off // es)
    rec = VG.vignette_rings_tensor(image, center=center, radius=radius, rings=case.rings, lo=lo, hi=hi)
    out = VG.apply_vignette_tensor(image, case.vignette(), center=center, radius=radius, out=image if case.inplace else None)
    wres, wrec = VC.reference_of(case)
    bad = int((rec.cpu().numpy() != wrec).sum()) + int((out.cpu().numpy() != wres).sum())
    bad += int((base_t.cpu().numpy() != VC.expected_base(case, wres)).sum())
    return desc, bad


def circle_remap_case(rng, dev) -> tuple[str, int]:
    h, w = int(rng.integers(24, 700)), int(rng.integers(24, 700))
    wo, ho = int(rng.integers(8, 600)), int(rng.integers(8, 600))
    interp = int(rng.choice([0, 1, 2, 4]))
    r = float(rng.uniform(0.2, 0.6) * min(h, w))
    cs = [(float(w / 2 + rng.uniform(-0.3, 0.3) * w), float(h / 2 + rng.uniform(-0.3, 0.3) * h)) for _ in range(2)]
    if rng.random() < 0.3:
        cs = [tuple(np.round(np.array(c) * 4) / 4) for c in cs]
    srcs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2)]
    t = V.EquirectangularEncoder() * V.FisheyeDecoder("equidistant")
    form = str(rng.choice(["apply one", "apply each", "lr one", "lr each"]))
    per = cs if form.endswith("each") else [cs[0], cs[0]]
    from vr180_convert_amd import remapper

    if form.startswith("apply"):
        got = V.apply(t, in_paths=srcs, radius=r, center=cs if form.endswith("each") else cs[0], size_output=(wo, ho), interpolation=interp, device=dev)
    else:
        sbs = V.apply_lr_tensors(t, torch.from_numpy(srcs[0]).to(dev), torch.from_numpy(srcs[1]).to(dev), radius=r,
                                 center=tuple(cs) if form.endswith("each") else cs[0], size_output=(wo, ho), interpolation=interp).cpu().numpy()
        got = [sbs[:, :wo], sbs[:, wo:]]
    bad = 0
    for g, s_, c in zip(got, srcs, per):
        xm, ym = remapper._host_map(t, radius=r, size_input=(h, w), size_output=(wo, ho), center=c)
        bad += int(neq(np.asarray(g), O.remap(s_, xm, ym, interp)).sum())
    return f"circle remap {form} {h}x{w} -> {wo}x{ho} interp {interp} radius {r!r} centres {cs} kinds {remapper.last_launch_kinds()}", bad


CIRCLE = {"drawn": 0}
CHROMA = {"drawn": 0, "fixup": 0, "literal": 0}


def chroma_case(rng, dev) -> tuple[str, int]:
    """--chroma: a remap case with a random ChromaticAberration (chromatic.py) against the per-channel oracle composition -- channel c
    of the result is channel c of the oracle's image for the chain with that channel's polynomial appended.  Coefficients within 2 %
    linear and 2 % cubic of the identity, now and then a constant term (the table of that channel then loses its centre: fix-up
    passes).  The ill-conditioned pixels and float32 rounding ties of each channel's own chain are left out and counted like one_case's."""
    from vr180_convert_amd import chromatic, remapper

    CHROMA["drawn"] += 1
    spec, rot_at = rand_spec(rng)
    h, w = rand_size(rng, 0.0, 2), rand_size(rng, 0.0, 2)
    wo, ho = rand_size(rng, 0.0), rand_size(rng, 0.0)
    interp = int(rng.choice([0, 1, 1, 2, 3, 4]))
    border = int(rng.integers(0, 6))
    bval = tuple(int(v) for v in rng.integers(0, 256, 3))
    radius = float(rng.uniform(0.25, 0.7) * min(h, w)) * (-1 if rng.random() < 0.05 else 1)
    n = int(rng.choice([1, 1, 2, 3]))

    def coefs():
        if rng.random() < 0.15:
            return None
        c = [0.0, 1.0 + float(rng.uniform(-0.02, 0.02)), 0.0, float(rng.uniform(-0.02, 0.02))]
        if rng.random() < 0.15:
            c[0] = float(rng.normal(0, 0.01))
        return c[:2] if rng.random() < 0.2 else c

    co = {"b": coefs(), "g": coefs() if rng.random() < 0.2 else None, "r": coefs()}
    ca = chromatic.ChromaticAberration(red=co["r"], blue=co["b"], green=co["g"])
    rots = None
    if rot_at is not None and n > 1 and rng.random() < 0.4:
        rots = [rand_rot(rng, rng.random() < 0.3) for _ in range(n)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
    fills = [rng.integers(0, 256, (ho, wo, 3), dtype=np.uint8) for _ in range(n)]
    srcs = [make_view(rng, im, dev, True) for im in imgs]
    dsts = [make_view(rng, f, dev, True) for f in fills]
    paths = V.remap_tensors(CS.to_product(spec), srcs, dsts, radius=radius, interpolation=interp, boarder_mode=border, boarder_value=bval,
                            chromatic=ca, **({} if rots is None else {"rotations": rots}))
    kinds = remapper.last_launch_kinds()
    for kd in kinds:
        KINDS[kd] = KINDS.get(kd, 0) + 1
    CHROMA["fixup"] += any(kd.endswith("+fixup") for kd in kinds)
    CHROMA["literal"] += "literal" in paths
    bad = 0
    for k in range(n):
        spec_k = spec if rots is None else spec[:rot_at] + [("rot", rots[k].tolist())] + spec[rot_at + 1:]
        got = dsts[k].cpu().numpy()
        for c, name in enumerate("bgr"):
            spec_c = spec_k + [("poly", list(ca.coefs(name)))] if ca.coefs(name) is not None else spec_k
            xm, ym = O.get_map(spec_c, radius=radius, size_input=(h, w), size_output=(wo, ho))
            want = O.remap(imgs[k], xm, ym, interp, border, bval, dst=fills[k].copy())[..., c]
            d = got[..., c] != want
            if d.any():
                ill = ill_conditioned(spec_c, radius, (h, w), (wo, ho))
                if border in (1, 2, 3, 4):  # (one_case's rule for the modes that read the source far outside; NaN counts as singular)
                    ill |= ~((np.abs(xm) < 2.0 ** 20) & (np.abs(ym) < 2.0 ** 20))
                SINGULAR[0] += int((d & ill).sum())
                d &= ~ill
            if d.any():
                tie = float32_ties(spec_c, radius, (h, w), (wo, ho))
                TIES[0] += int((d & tie).sum())
                d &= ~tie
            if d.any() and DUMP[0]:
                jj, ii = np.argwhere(d)[0]
                print(f"  unit {k} channel {name}: {int(d.sum())} bytes differ, first (row {jj}, col {ii}) map=({xm[jj, ii]!r}, {ym[jj, ii]!r}) "
                      f"got={int(got[jj, ii, c])} want={int(want[jj, ii])}")
            bad += int(d.sum())
    return (f"chroma spec={spec} {co} {h}x{w} -> {wo}x{ho} x{n} interp {interp} border {border} bval {bval} radius {radius!r} "
            f"rots={'per unit' if rots is not None else 'no'} paths {paths} kinds {kinds}"), bad


def feat_draw(rng) -> dict:
    """the draws of feat_case's detect half that decide whether v1c_feat_detect refuses the case: no image, no device (tests/test_feat_host.py
    runs feat_ref.refusal over thousands of them).  Nine in ten sizes are drawn so that the working image reaches 34 pixels, nine in ten
    margins so that radius * scale - margin stays at 2 or more: the rest may be refused (a working image under 33 x 33, an empty circle)"""
    kind = FEAT_IMAGES[int(rng.integers(len(FEAT_IMAGES)))]
    scale = [1.0, 0.5, 1 / 3, float(rng.uniform(0.2, 1.0))][int(rng.integers(4))]
    lo = max(40, int(np.ceil(34 / scale))) if rng.random() < 0.9 else 40
    h, w = int(rng.integers(lo, 701)), int(rng.integers(lo, 701))
    if kind == "sphere":  # (sphere_scene.render: square, and seconds above a few hundred pixels)
        h = w = min(h, w, 320)
    cn = int(rng.choice([1, 3, 4]))
    radius = float(rng.uniform(0.2, 1.5) * min(h, w) / 2)
    margin = int(rng.integers(0, 41))
    if rng.random() < 0.9:
        margin = min(margin, max(0, int(radius * scale) - 2))
    return {"kind": kind, "h": h, "w": w, "cn": cn, "gray2d": bool(cn == 1 and rng.random() < 0.3), "scale": scale, "radius": radius,
            "margin": margin, "fast_threshold": int(rng.choice([1, 5, 20, 60, 255], p=[0.2, 0.25, 0.3, 0.2, 0.05])),
            "cell": int(rng.choice([8, 16, 32, 47, 64])), "per_cell": int(rng.integers(1, 5)),
            "max_keypoints": int(rng.choice([1, 7, 100, 8192, 65536], p=[0.1, 0.1, 0.2, 0.35, 0.25]))}  # (mostly cases with keypoints to match)


def feat_image(rng, kind: str, h: int, w: int, cn: int) -> np.ndarray:
    """(h, w, cn) uint8: a noise disc on black, uniform noise, low-contrast noise (0..30), filled polygons, discs and blobs on a gradient
    (flat regions: corners of repeated scores), a rendered sphere scene, or a flat image (no keypoint)"""
    if kind == "disc":
        from vr180_convert_amd.synth import noise_disc

        return noise_disc(h, w, int(rng.integers(1000)), cn=cn)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, cn), dtype=np.uint8)
    if kind == "low":
        return rng.integers(0, 31, (h, w, cn), dtype=np.uint8)
    if kind == "flat":
        return np.full((h, w, cn), int(rng.integers(0, 256)), np.uint8)
    if kind == "sphere":
        import sphere_scene as S

        g = S.render(h, S.rotation(rng.normal(0, 1, 3), float(rng.uniform(0, 20))))[..., :1]
        return np.ascontiguousarray(np.concatenate([g, g, g, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=2)[..., :cn])
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    a = 60 + 80 * (xx * rng.uniform(0, 1) / w + yy * rng.uniform(0, 1) / h)
    for _ in range(int(rng.integers(3, 40))):
        if rng.random() < 0.7:  # a filled triangle: inside iff on one side of all three edges
            px, py = rng.uniform(-0.1 * w, 1.1 * w, 3), rng.uniform(-0.1 * h, 1.1 * h, 3)
            e = [(px[(k + 1) % 3] - px[k]) * (yy - py[k]) - (py[(k + 1) % 3] - py[k]) * (xx - px[k]) for k in range(3)]
            m = ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))
            a[m] = float(rng.choice([0, 40, 40, 200, 200, 255]))
        elif rng.random() < 0.5:  # a filled disc
            a[(xx - rng.uniform(0, w)) ** 2 + (yy - rng.uniform(0, h)) ** 2 <= rng.uniform(2, 30) ** 2] = float(rng.integers(0, 256))
        else:  # a Gaussian blob
            a += rng.uniform(-120, 120) * np.exp(-((xx - rng.uniform(0, w)) ** 2 + (yy - rng.uniform(0, h)) ** 2) / (2 * rng.uniform(1.5, 12) ** 2))
    g = np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(g[..., None], cn, axis=2))


def feat_sets(rng) -> tuple[np.ndarray, np.ndarray]:
    """two random descriptor sets with near copies (matches), exact duplicates and ties planted; sizes on the matcher's tile of 256"""
    def size():
        return int(rng.choice([0, 1, 255, 256, 257])) if rng.random() < 0.4 else int(np.exp(rng.uniform(np.log(300), np.log(20000))))

    na, nb = size(), size()
    a = rng.integers(0, 256, (na, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    if na and nb:
        k = (min(na, nb) + 2) // 3
        a[:k] = b[rng.integers(0, nb, k)] ^ rng.integers(0, 2, (k, 32), dtype=np.uint8)  # up to 32 bits off a candidate
        for _ in range(int(rng.integers(0, 6))):  # exact duplicates among the candidates, a query equal to them / one bit off them
            j1, j2, i = int(rng.integers(nb)), int(rng.integers(nb)), int(rng.integers(na))
            b[j2] = b[j1]
            a[i] = b[j1]
            a[i, 0] ^= int(rng.integers(0, 2))
        for _ in range(int(rng.integers(0, 4))):  # ... and among the queries
            a[int(rng.integers(na))] = a[int(rng.integers(na))]
    return a, b


def _differing(got, want) -> int:
    """differing elements of two tuples of arrays; an array of another shape counts whole"""
    return sum(int((np.asarray(g) != np.asarray(w)).sum()) if np.shape(g) == np.shape(w) else max(np.size(g), np.size(w), 1)
               for g, w in zip(got, want))


def feat_case(rng, dev) -> tuple[str, int, bool]:
    """the feature pipeline (v1c_feat_detect / v1c_feat_match through features.detect / features.match) against tests/feat_ref.py, every
    array equal, shapes included: images of six kinds in a random view with random parameters off the defaults; the matcher on the
    descriptors of two such detects (the second image: the first one rolled a few pixels under a little noise, or an independent one), or,
    a third of the time, on random descriptor sets of 0 ... 20000 entries with planted copies, duplicates and ties.  Returns (description,
    differing elements, counted): a refusal of the product that feat_ref.refusal predicts is correct and does not count as a case."""
    import feat_ref as R
    from vr180_convert_amd import features as F

    p = feat_draw(rng)
    kind, h, w, cn = p["kind"], p["h"], p["w"], p["cn"]
    kw = {k: p[k] for k in ("margin", "fast_threshold", "cell", "per_cell", "max_keypoints")}
    img = feat_image(rng, kind, h, w, cn)
    sets = rng.random() < 0.33
    mkw = {"max_distance": int(rng.choice([0, 16, 64, 256])), "ratio": FEAT_RATIOS[int(rng.integers(len(FEAT_RATIOS)))]}
    imgs = [img]
    if not sets:
        if rng.random() < 0.6:
            dy, dx = (int(v) for v in rng.integers(-6, 7, 2))
            second = np.roll(img, (dy, dx), axis=(0, 1)).astype(np.int16) + rng.integers(-3, 4, img.shape)
            imgs.append(np.clip(second, 0, 255).astype(np.uint8))
            how = f"rolled ({dy},{dx}) + noise"
        else:
            imgs.append(feat_image(rng, kind, h, w, cn))
            how = "independent"
    desc = (f"FEAT image={kind} size=({w},{h}) cn={'2-D' if p['gray2d'] else cn} scale={p['scale']!r} radius={p['radius']!r} "
            + " ".join(f"{k}={v}" for k, v in kw.items()))
    FEAT["drawn"] += 1
    why = R.refusal(h, w, p["scale"], p["radius"], p["margin"])
    bad, descs = 0, []
    for k, im in enumerate(imgs):
        t = make_view(rng, im, dev, allow_unaligned=True)
        desc += f" view{k}: contiguous={t.is_contiguous()} byte offset={t.storage_offset()}"
        if p["gray2d"]:
            t, im = t[..., 0], im[..., 0]
        try:
            got = F.detect(t, radius=p["radius"], scale=p["scale"], **kw)
        except ValueError:
            if why is None:
                raise
            FEAT["refused"] += 1
            return desc + f" (refused as predicted: {why})", 0, False
        if why is not None:
            return desc + f" (NOT refused; predicted: {why})", 1, True
        want = R.detect(im, radius=p["radius"], scale=p["scale"], **kw)
        bad += _differing(got, want)
        descs.append(want[1])
        desc += f" n{k}={len(want[0])}"
    if sets:
        descs = list(feat_sets(rng))
        desc += " match on random sets"
    else:
        desc += f" second image {how}"
    na, nb = len(descs[0]), len(descs[1])
    desc += f" match {na} x {nb} {mkw!r}"
    got = F.match(descs[0], descs[1], **mkw)
    want = (R.match_blocked if max(na, nb) > 4096 else R.match)(descs[0], descs[1], **mkw)
    bad += _differing(got, want)
    KINDS["feat"] = KINDS.get("feat", 0) + 1
    return desc + f" matches={len(want[0])}", bad, True


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--big", type=float, default=0.15, help="share of sizes drawn from 1200 - 2700")
    ap.add_argument("--lut", type=float, default=0.15, help="share of cases that fuzz cv2.remap alone (v1c_remap_lut) on random maps")
    ap.add_argument("--hot", type=float, default=0.3, help="share of the chain cases drawn from the shapes the tuned kernels are selected for")
    ap.add_argument("--gen2", type=float, default=0.0, help="share of the chain cases with radial stages / zooms in front of a rotation (general mode 2)")
    ap.add_argument("--api", type=float, default=0.1, help="share of cases through apply() / apply_lr() on host arrays")
    ap.add_argument("--auto", type=float, default=0.06, help="share of cases through apply_lr_tensors(radius='auto') with the radius on the device")
    ap.add_argument("--fused", type=float, default=0.06, help="share of cases through v1c_remap_fused by raw ctypes")
    ap.add_argument("--wide", type=float, default=0.0, help="share of cases with uint16 / float32 pixels: the chain cases and the LUT cases (k_remap_wide) against wide_ref.remap")
    ap.add_argument("--png", type=float, default=0.0, help="share of cases through the device PNG encoder (encode_png_tensor) against png_ref.encode")
    ap.add_argument("--jpeg", type=float, default=0.0, help="share of cases through the device JPEG encoder (encode_jpeg_tensor) against jpg_ref.encode")
    ap.add_argument("--jpegdec", type=float, default=0.0, help="share of cases through the device JPEG decoder (decode_jpeg_tensor) against jpgdec_ref.decode")
    ap.add_argument("--jpegbatch", type=float, default=0.0, help="share of cases through the batched device JPEG encoder (encode_jpeg_tensors) against the single calls and jpg_ref.encode")
    ap.add_argument("--jpegopt", type=float, default=0.0, help="share of cases through the device JPEG encoder with optimised Huffman tables (optimize=True, single and batched) against jpg_opt_ref.encode")
    ap.add_argument("--jpegprog", type=float, default=0.0, help="share of cases through the device decoder of progressive JPEG files (decode_jpeg_tensor(progressive=True)) against jpgprog_ref.decode")
    ap.add_argument("--jpegxc", type=float, default=0.0, help="share of cases through the lossless JPEG transcoder (transcode_regions: crops, splits, swaps) against jpgxc_ref.transcode")
    ap.add_argument("--jpegxf", type=float, default=0.0, help="share of cases through the lossless JPEG composer (compose_regions: joins, rotations, flips of up to four files) against jpgxf_ref.compose")
    ap.add_argument("--jpegdmg", type=float, default=0.0, help="share of cases through the device JPEG decoders with one random damage inside a scan, against the verdict of tests/jpgdmg_cases.py")
    ap.add_argument("--jpegodd", type=float, default=0.0, help="share of cases through the device JPEG decoders with a legal file of unusual structure or one damaged header, against tests/jpgodd_cases.py")
    ap.add_argument("--circle", type=float, default=0.0, help="share of cases through the image-circle fit (v1c_fit_circle) against circle_ref.fit, a part of them remaps with random off-centre center= against the oracle")
    ap.add_argument("--colormatch", type=float, default=0.0, help="share of cases through the colour match of two eyes (color_match_luts_tensor, apply_luts_tensor) against colormatch_ref, byte for byte")
    ap.add_argument("--vignette", type=float, default=0.0, help="share of cases through the vignetting correction (vignette_rings_tensor, apply_vignette_tensor) against vignette_ref, byte for byte")
    ap.add_argument("--chroma", type=float, default=0.0, help="share of the remap (chain) cases that draw a ChromaticAberration (remap_tensors(chromatic=)) and are held to the per-channel oracle composition")
    ap.add_argument("--cases", type=int, default=None, help="stop after this many cases (before --seconds runs out)")
    ap.add_argument("--feat", type=float, default=0.0, help="share of cases through the feature pipeline (features.detect / features.match) against tests/feat_ref.py")
    ap.add_argument("--only", type=int, default=None, help="run only this case number (reproduce)")
    ap.add_argument("--log", default=None)
    ap.add_argument("--trace", default=None, help="file that always holds the number of the case being run")
    ap.add_argument("--dump", action="store_true", help="print where a mismatching unit differs")
    a = ap.parse_args()
    DUMP[0] = a.dump
    HOT[0] = a.hot
    GEN2[0] = a.gen2
    dev = torch.device("cuda", 0)
    log = open(a.log, "a") if a.log else None

    def say(s: str) -> None:
        print(s, flush=True)
        if log:
            log.write(s + "\n")
            log.flush()

    t0 = time.time()
    n_cases = n_bad = 0
    last = t0
    case = 0
    while time.time() - t0 < a.seconds and (a.cases is None or case < a.cases):
        rng = np.random.default_rng([a.seed, case])  # every case reproducible by itself
        if a.only is not None:
            rng = np.random.default_rng([a.seed, a.only])
        if a.trace:  # (a crash of the process -- a GPU memory fault aborts it -- leaves the case that was running on record)
            with open(a.trace, "w") as tf:
                tf.write(f"seed {a.seed} case {a.only if a.only is not None else case}\n")
        try:
            r_kind = rng.random()
            wide_chain = False
            counted = True
            rest00000 = 1.0 - a.vignette
            rest0000 = rest00000 - a.colormatch
            rest000 = rest0000 - a.circle
            rest00 = rest000 - a.jpegodd
            rest0 = rest00 - a.jpegdmg
            rest = rest0 - a.jpegxf
            top = rest - a.jpegxc - a.jpegprog - a.jpegopt - a.jpegbatch - a.jpegdec
            if r_kind >= rest00000:  # (the new shares come off the top: with all of them at 0 every earlier seed replays as it ran)
                desc, bad = vignette_case(rng, dev)
            elif r_kind >= rest0000:
                desc, bad = colormatch_case(rng, dev)
            elif r_kind >= rest000:
                desc, bad = circle_case(rng, dev)
            elif r_kind >= rest00:
                desc, bad = jpegodd_case(rng, dev)
            elif r_kind >= rest0:
                desc, bad = jpegdmg_case(rng, dev)
            elif r_kind >= rest:
                desc, bad = jpegxf_case(rng, dev)
            elif r_kind >= rest - a.jpegxc:
                desc, bad = jpegxc_case(rng, dev)
            elif r_kind >= rest - a.jpegxc - a.jpegprog:
                desc, bad = jpegprog_case(rng, dev)
            elif r_kind >= rest - a.jpegxc - a.jpegprog - a.jpegopt:
                desc, bad = jpegopt_case(rng, dev)
            elif r_kind >= rest - a.jpegxc - a.jpegprog - a.jpegopt - a.jpegbatch:
                desc, bad = jpegbatch_case(rng, dev)
            elif r_kind >= top:
                desc, bad = jpegdec_case(rng, dev)
            elif r_kind >= top - a.feat:
                desc, bad, counted = feat_case(rng, dev)
            elif r_kind >= top - a.feat - a.png:
                desc, bad = png_case(rng, dev)
            elif r_kind >= top - a.feat - a.png - a.jpeg:
                desc, bad = jpeg_case(rng, dev)
            elif r_kind >= top - a.feat - a.png - a.jpeg - a.wide:
                dtype = np.uint16 if rng.random() < 0.5 else np.float32
                if rng.random() < 0.3:
                    desc, bad = lut_case(rng, dev, dtype)
                else:
                    wide_chain = True
                    desc, bad = one_case(rng, dev, a.big, dtype)
            elif r_kind < a.lut:
                desc, bad = lut_case(rng, dev)
            elif r_kind < a.lut + 0.05:
                desc, bad = radius_case(rng, dev)
            elif r_kind < a.lut + 0.05 + a.api:
                desc, bad = api_case(rng, dev)
            elif r_kind < a.lut + 0.05 + a.api + a.auto:
                desc, bad = auto_case(rng, dev)
            elif r_kind < a.lut + 0.05 + a.api + a.auto + a.fused:
                desc, bad = fused_case(rng, dev)
            elif a.chroma > 0 and rng.random() < a.chroma:  # (no draw when the option is off: earlier seeds replay as they ran)
                desc, bad = chroma_case(rng, dev)
            else:
                desc, bad = one_case(rng, dev, a.big)
        except Exception as e:  # noqa: BLE001 -- a refusal of the product (documented limits) is reported, not fatal
            desc, bad, counted = f"EXCEPTION {type(e).__name__}: {e}", -1, True
        n_cases += 1 if counted else 0
        if wide_chain and bad >= 0:
            WIDE_CHAIN["run"] += 1
            if LAST_MASKED[0] > 0.05:  # mostly masks, little comparison: checked like every case, but not a case of the run's total
                WIDE_CHAIN["not counted"] += 1
                n_cases -= 1
        if bad != 0:
            n_bad += 1
            say(f"[case {a.only if a.only is not None else case}] {'MISMATCH ' + str(bad) + ' bytes' if bad > 0 else ''} {desc}")
        if a.only is not None:
            say(f"case {a.only}: {bad} differing bytes; {desc}")
            break
        case += 1
        if time.time() - last > 30:
            last = time.time()
            say(f"... {n_cases} cases, {n_bad} reported, {time.time() - t0:.0f} s")
    say(f"fuzz seed {a.seed}: {n_cases} cases in {time.time() - t0:.0f} s, {n_bad} reported; {SINGULAR[0]} differing ill-conditioned pixels left out"
        + (f", {TIES[0]} at float32 rounding ties" if TIES[0] else "")
        + (f"; wide chain cases: {WIDE_CHAIN['run']} run, {WIDE_CHAIN['not counted']} of them over 5 % masked and not counted, "
           f"{WIDE_CHAIN['masked px']} of {WIDE_CHAIN['px']} pixels masked" if WIDE_CHAIN["run"] else "")
        + (f"; feat cases: {FEAT['drawn']} drawn, {FEAT['refused']} of them refused as predicted and not counted" if FEAT["drawn"] else "")
        + (f"; jpegxf cases: {XF['drawn']} drawn, {XF['refused']} of them refused by both sides alike" if XF["drawn"] else "")
        + (f"; jpegdmg cases: {DMG['drawn']} drawn, {DMG['refused']} refused by the last pass, {DMG['decoded']} decoded, {DMG['parse']} left to the parse"
           if DMG["drawn"] else "")
        + (f"; jpegodd cases: {ODD['drawn']} drawn, {ODD['legal']} legal files and {ODD['damage']} damaged headers, {ODD['refused']} of them refused as predicted"
           if ODD["drawn"] else "")
        + (f"; circle cases: {CIRCLE['drawn']} drawn" if CIRCLE["drawn"] else "")
        + (f"; colormatch cases: {COLORMATCH['drawn']} drawn" if COLORMATCH["drawn"] else "")
        + (f"; vignette cases: {VIGNETTE['drawn']} drawn" if VIGNETTE["drawn"] else "")
        + (f"; chroma cases: {CHROMA['drawn']} drawn, {CHROMA['fixup']} with a fix-up pass, {CHROMA['literal']} on the literal path" if CHROMA["drawn"] else ""))
    say("kernel families of the chain cases' launch groups: " + ", ".join(f"{k} x{v}" for k, v in sorted(KINDS.items())))
    return 1 if n_bad else 0


if __name__ == "__main__":
    sys.exit(main())
