"""The entry of the pair mirror kernel's tap table (csrc/tap_table.hpp) without a GPU.

plan.hip keeps, for a pair plan without rest tiles, the fixed-point tap coordinates of every lane: 12 bytes holding x, y and the
mirrored row's y of the lane's 4 pixels, each as a 12-bit base and three deltas (7 bits unsigned for x, 6 bits signed for y).
k_ray_lin3_pair_mirror_seq_tab decodes what k_fill_tap_table encoded, so the kernel's bytes depend on decode(encode(c)) == c for
every c that fits -- and on fits() refusing everything else, because a plan whose map does not fit keeps no table.  These tests hold
the product's own functions, compiled for the host (tests/host_tap_table), to that:

* the packed size is 12 bytes;
* round trip of random in-range values and of every field's extremes, alone and combined;
* fits() is false one step outside each range, for every pixel position of every field;
* the bit layout documented in the header (a decoder written here from that comment reads the same values);
* the same walk as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "host_tap_table" / "tap.cpp"


@pytest.fixture(scope="module")
def tap_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_tap_table") / "libv1c_tap_table.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(out), str(HARNESS)], check=True,
                   capture_output=True, timeout=300)
    lib = C.CDLL(str(out))
    vp = C.c_void_p
    lib.tap_limits.argtypes = [vp]
    lib.tap_many.argtypes = [vp, C.c_int64, vp, vp, vp]
    lib.tap_decode.argtypes = [vp, vp]
    return lib


@pytest.fixture(scope="module")
def limits(tap_lib):
    v = np.zeros(5, np.int32)
    tap_lib.tap_limits(v.ctypes.data)
    base_max, dx_max, dy_min, dy_max, px = (int(x) for x in v)
    return base_max, dx_max, dy_min, dy_max, px


def run_many(lib, coords):
    coords = np.ascontiguousarray(coords, np.int32).reshape(-1, 12)
    n = len(coords)
    fit = np.zeros(n, np.uint8)
    words = np.zeros((n, 3), np.uint32)
    back = np.zeros((n, 12), np.int32)
    lib.tap_many(coords.ctypes.data, n, fit.ctypes.data, words.ctypes.data, back.ctypes.data)
    return fit.astype(bool), words, back


def from_deltas(base, d):
    """(n, 3) bases and (n, 3, 3) deltas -> (n, 12) coordinates x[4] | y[4] | y2[4]"""
    base, d = np.asarray(base, np.int64), np.asarray(d, np.int64)
    c = np.concatenate([base[:, :, None], base[:, :, None] + np.cumsum(d, axis=2)], axis=2)
    return c.reshape(len(base), 12)


def test_packed_size_and_limits(tap_lib, limits):
    assert tap_lib.tap_sizeof() == 12
    # 12-bit bases, 7-bit unsigned x steps, 6-bit signed y steps, 4 pixels per lane: 3 * 12 + 3 * 7 + 6 * 6 = 93 bits of the 96
    assert limits == (4095, 127, -32, 31, 4)


def test_round_trip_of_random_in_range_values(tap_lib, limits):
    base_max, dx_max, dy_min, dy_max, _ = limits
    rng = np.random.default_rng(20261021)
    n = 400_000
    base = rng.integers(0, base_max + 1, (n, 3))
    d = np.empty((n, 3, 3), np.int64)
    d[:, 0] = rng.integers(0, dx_max + 1, (n, 3))
    d[:, 1:] = rng.integers(dy_min, dy_max + 1, (n, 2, 3))
    coords = from_deltas(base, d)
    fit, words, back = run_many(tap_lib, coords)
    assert fit.all()
    assert np.array_equal(back, coords)
    assert not (words[:, 1] >> 31).any() and not (words[:, 2] >> 30).any()  # the spare bits stay zero


def test_round_trip_of_every_fields_extremes(tap_lib, limits):
    base_max, dx_max, dy_min, dy_max, _ = limits
    lo = np.array([[0, 0, 0], [0, dy_min, dy_min]])   # (base, delta) minima of x | y | y2 ...
    hi = np.array([[base_max] * 3, [dx_max, dy_max, dy_max]])
    cases = []
    # every one of the 12 fields at its minimum and at its maximum while the others sit mid-range, then all corners of (bases, deltas)
    mid_base, mid_d = np.array([2048, 2048, 2048]), np.array([[32, 32, 32], [0, 0, 0], [0, 0, 0]])
    for f in range(3):
        for ext in (lo, hi):
            b = mid_base.copy()
            b[f] = ext[0][f]
            cases.append((b, mid_d))
            for k in range(3):
                d = mid_d.copy()
                d[f, k] = ext[1][f]
                cases.append((mid_base, d))
    for bx in (0, base_max):
        for by in (0, base_max):
            for dx in (0, dx_max):
                for dy in (dy_min, dy_max):
                    for dy2 in (dy_min, dy_max):
                        cases.append((np.array([bx, by, by]), np.array([[dx] * 3, [dy] * 3, [dy2] * 3])))
    coords = from_deltas(np.array([c[0] for c in cases]), np.array([c[1] for c in cases]))
    fit, _, back = run_many(tap_lib, coords)
    assert fit.all()
    assert np.array_equal(back, coords)


def test_fits_is_false_one_step_outside_each_range(tap_lib, limits):
    base_max, dx_max, dy_min, dy_max, _ = limits
    mid_base, mid_d = np.array([2048, 2048, 2048]), np.array([[32, 32, 32], [0, 0, 0], [0, 0, 0]])
    inside, outside = [], []
    d_lo, d_hi = [0, dy_min, dy_min], [dx_max, dy_max, dy_max]
    for f in range(3):
        for edge, step in ((0, -1), (base_max, 1)):
            b = mid_base.copy()
            b[f] = edge
            inside.append((b, mid_d))
            b = b.copy()
            b[f] += step
            outside.append((b, mid_d))
        for k in range(3):
            for edge, step in ((d_lo[f], -1), (d_hi[f], 1)):
                d = mid_d.copy()
                d[f, k] = edge
                inside.append((mid_base, d))
                d = d.copy()
                d[f, k] += step
                outside.append((mid_base, d))
    assert len(outside) == 3 * 2 + 3 * 3 * 2
    fit_in, _, _ = run_many(tap_lib, from_deltas(np.array([c[0] for c in inside]), np.array([c[1] for c in inside])))
    fit_out, _, _ = run_many(tap_lib, from_deltas(np.array([c[0] for c in outside]), np.array([c[1] for c in outside])))
    assert fit_in.all()
    assert not fit_out.any()


def test_the_words_follow_the_documented_layout(tap_lib, limits):
    """A decoder written from tap_table.hpp's comment, on random fitting entries; and tap_decode on words built here."""
    base_max, dx_max, dy_min, dy_max, _ = limits
    rng = np.random.default_rng(7)
    n = 50_000
    base = rng.integers(0, base_max + 1, (n, 3))
    d = np.empty((n, 3, 3), np.int64)
    d[:, 0] = rng.integers(0, dx_max + 1, (n, 3))
    d[:, 1:] = rng.integers(dy_min, dy_max + 1, (n, 2, 3))
    coords = from_deltas(base, d)
    _, words, _ = run_many(tap_lib, coords)
    w = words.astype(np.int64)

    def sext6(v):
        return ((v & 63) ^ 32) - 32

    x0 = w[:, 0] & 4095
    dx = np.stack([(w[:, 0] >> 12) & 127, (w[:, 0] >> 19) & 127, ((w[:, 0] >> 26) & 63) | (((w[:, 1] >> 30) & 1) << 6)], axis=1)
    y0, y20 = w[:, 1] & 4095, w[:, 2] & 4095
    dy = np.stack([sext6(w[:, 1] >> s) for s in (12, 18, 24)], axis=1)
    dy2 = np.stack([sext6(w[:, 2] >> s) for s in (12, 18, 24)], axis=1)
    assert np.array_equal(np.stack([x0, y0, y20], axis=1), base)
    assert np.array_equal(np.stack([dx, dy, dy2], axis=1), d)
    # the product's decoder on words assembled here
    one = np.array([100 | 5 << 12 | 127 << 19 | (77 & 63) << 26, 4095 | (-32 & 63) << 12 | 31 << 18 | (-1 & 63) << 24 | (77 >> 6) << 30,
                    7 | 0 << 12 | (-13 & 63) << 18 | 13 << 24], np.uint32)
    back = np.zeros(12, np.int32)
    tap_lib.tap_decode(one.ctypes.data, back.ctypes.data)
    assert back.tolist() == [100, 105, 232, 309, 4095, 4063, 4094, 4093, 7, 7, -6, 7]


def test_stand_alone_walk_under_the_sanitizers(tmp_path):
    """The same header in a program of its own (tests/host_tap_table/tap.cpp -DTAP_MAIN), built with AddressSanitizer and UBSan:
    extremes of every field, 200 000 pseudo-random entries, and the encoder on values that do not fit."""
    exe = tmp_path / "tap_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DTAP_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-o", str(exe), str(HARNESS)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ", 0 bad" in r.stdout
