"""The compact entry of the pair mirror kernel's tap table (csrc/tap_table.hpp: TapEntry8) without a GPU.

Where a plan's 12-byte table would be large, plan.hip keeps 8 bytes per lane: x and y of the lane's 4 pixels as a 12-bit base, a first
step (10 bits, unsigned for x, signed for y) and two second differences (3 bits signed each), and -- instead of the mirrored row's y2 --
e[k] = y2[k] - (K - y[k]), 2 bits signed per pixel, with K one number per tile pair.  k_ray_lin3_pair_mirror_seq_tab8 decodes what
k_fill_tap_table encoded, so the kernel's bytes depend on decode(encode(c, K), K) == c for every c that fits and on fits() refusing
everything else.  These tests hold the product's own functions, compiled for the host (tests/host_tap_table/tap8.cpp), to that:

* the packed size is 8 bytes;
* round trip of random in-range values and of every field's extremes, alone and combined;
* fits() is false one step outside each range, for every field and pixel position (e = -3 and 2, second differences -5 and 4);
* the bit layout documented in the header (a decoder written here from that comment reads the same values);
* coordinates that fit both forms decode to the same twelve numbers through the 12-byte entry and through the compact one;
* the same walk as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "host_tap_table" / "tap8.cpp"


@pytest.fixture(scope="module")
def tap_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_tap_table8") / "libv1c_tap_table8.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(out), str(HARNESS)], check=True,
                   capture_output=True, timeout=300)
    lib = C.CDLL(str(out))
    vp = C.c_void_p
    lib.tap8_limits.argtypes = [vp]
    lib.tap8_many.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp]
    lib.tap8_decode_words.argtypes = [vp, C.c_int, vp]
    return lib


@pytest.fixture(scope="module")
def limits(tap_lib):
    v = np.zeros(9, np.int32)
    tap_lib.tap8_limits(v.ctypes.data)
    return tuple(int(x) for x in v)


def run_many(lib, coords, K):
    coords = np.ascontiguousarray(coords, np.int32).reshape(-1, 12)
    n = len(coords)
    K = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.int32), (n,)))
    fit, fit12 = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    words = np.zeros((n, 2), np.uint32)
    back, back12 = np.zeros((n, 12), np.int32), np.zeros((n, 12), np.int32)
    lib.tap8_many(coords.ctypes.data, K.ctypes.data, n, fit.ctypes.data, words.ctypes.data, back.ctypes.data, fit12.ctypes.data,
                  back12.ctypes.data)
    return fit.astype(bool), words, back, fit12.astype(bool), back12


def from_fields(x0, dx1, ddx, y0, dy1, ddy, e, K):
    """the entry's fields -- (n,) bases and first steps, (n, 2) second differences, (n, 4) e, (n,) K -- -> (n, 12) coordinates
    x[4] | y[4] | y2[4]"""
    def axis(v0, d1, dd):
        v0, d1, dd = np.asarray(v0, np.int64), np.asarray(d1, np.int64), np.asarray(dd, np.int64)
        d = np.stack([d1, d1 + dd[:, 0], d1 + dd[:, 0] + dd[:, 1]], axis=1)
        return np.concatenate([v0[:, None], v0[:, None] + np.cumsum(d, axis=1)], axis=1)

    x, y = axis(x0, dx1, ddx), axis(y0, dy1, ddy)
    y2 = np.asarray(K, np.int64)[:, None] - y + np.asarray(e, np.int64)
    return np.concatenate([x, y, y2], axis=1)


def random_fields(rng, n, limits, dx_max=None, dy_lim=None):
    base_max, dx1_max, dy_min, dy_max, dd_min, dd_max, e_min, e_max, _ = limits
    dx_hi = dx1_max if dx_max is None else dx_max
    dy_lo, dy_hi = (dy_min, dy_max) if dy_lim is None else dy_lim
    return dict(x0=rng.integers(0, base_max + 1, n), dx1=rng.integers(0, dx_hi + 1, n), ddx=rng.integers(dd_min, dd_max + 1, (n, 2)),
                y0=rng.integers(0, base_max + 1, n), dy1=rng.integers(dy_lo, dy_hi + 1, n), ddy=rng.integers(dd_min, dd_max + 1, (n, 2)),
                e=rng.integers(e_min, e_max + 1, (n, 4)), K=rng.integers(-100_000, 400_000, n))


MID = dict(x0=2048, dx1=32, ddx=(0, 0), y0=2048, dy1=0, ddy=(0, 0), e=(0, 0, 0, 0), K=4711)


def cases_to_coords(cases):
    f = {k: np.array([c[k] for c in cases]) for k in MID}
    return from_fields(**f), f["K"]


def field_edges(limits):
    """(field, position or None, minimum, maximum) of every field of the entry"""
    base_max, dx1_max, dy_min, dy_max, dd_min, dd_max, e_min, e_max, _ = limits
    out = [("x0", None, 0, base_max), ("y0", None, 0, base_max), ("dx1", None, 0, dx1_max), ("dy1", None, dy_min, dy_max)]
    out += [(f, k, dd_min, dd_max) for f in ("ddx", "ddy") for k in range(2)]
    out += [("e", k, e_min, e_max) for k in range(4)]
    return out


def with_field(f, k, v):
    c = dict(MID)
    if k is None:
        c[f] = v
    else:
        t = list(c[f])
        t[k] = v
        c[f] = tuple(t)
    return c


def test_packed_size_and_limits(tap_lib, limits):
    assert tap_lib.tap8_sizeof() == 8
    # 2 x (12-bit base + 10-bit first step + 2 x 3-bit second differences) + 4 x 2 bits of e = 64 bits; the format asked for at least
    # 7 unsigned bits of dx1 and 6 signed bits of dy1
    assert limits == (4095, 1023, -512, 511, -4, 3, -2, 1, 4)
    assert 2 * (12 + 10 + 2 * 3) + 4 * 2 == 64


def test_round_trip_of_random_in_range_values(tap_lib, limits):
    rng = np.random.default_rng(20261021)
    f = random_fields(rng, 400_000, limits)
    coords = from_fields(**f)
    fit, _, back, _, _ = run_many(tap_lib, coords, f["K"])
    assert fit.all()
    assert np.array_equal(back, coords)


def test_round_trip_of_every_fields_extremes(tap_lib, limits):
    base_max, dx1_max, dy_min, dy_max, dd_min, dd_max, e_min, e_max, _ = limits
    cases = []
    for f, k, lo, hi in field_edges(limits):  # every field at its minimum and at its maximum while the others sit mid-range
        cases += [with_field(f, k, lo), with_field(f, k, hi)]
    for b in (0, base_max):  # all corners combined
        for dx in (0, dx1_max):
            for dy in (dy_min, dy_max):
                for dd in (dd_min, dd_max):
                    for e in (e_min, e_max):
                        for K in (-70_000, 0, 262_144):
                            cases.append(dict(x0=b, dx1=dx, ddx=(dd, dd), y0=b, dy1=dy, ddy=(dd, dd), e=(e,) * 4, K=K))
    coords, K = cases_to_coords(cases)
    fit, _, back, _, _ = run_many(tap_lib, coords, K)
    assert fit.all()
    assert np.array_equal(back, coords)


def test_fits_is_false_one_step_outside_each_range(tap_lib, limits):
    inside, outside = [], []
    for f, k, lo, hi in field_edges(limits):
        inside += [with_field(f, k, lo), with_field(f, k, hi)]
        outside += [with_field(f, k, lo - 1), with_field(f, k, hi + 1)]
    assert len(outside) == 2 * (4 + 4 + 4)
    # (among them: e = -3 and e = 2 at each of the 4 pixels, second differences -5 and 4 at both positions of x and of y)
    assert sum(1 for c in outside if -3 in c["e"]) == 4 and sum(1 for c in outside if 2 in c["e"]) == 4
    assert sum(1 for c in outside if -5 in c["ddx"] + c["ddy"]) == 4 and sum(1 for c in outside if 4 in c["ddx"] + c["ddy"]) == 4
    fit_in = run_many(tap_lib, *cases_to_coords(inside))[0]
    fit_out = run_many(tap_lib, *cases_to_coords(outside))[0]
    assert fit_in.all()
    assert not fit_out.any()


def test_the_words_follow_the_documented_layout(tap_lib, limits):
    """A decoder written from tap_table.hpp's comment, on random fitting entries; and tap8_decode on words built here."""
    rng = np.random.default_rng(7)
    f = random_fields(rng, 50_000, limits)
    coords = from_fields(**f)
    _, words, _, _, _ = run_many(tap_lib, coords, f["K"])
    w = words.astype(np.int64)

    def sext(v, bits):
        m = 1 << (bits - 1)
        return ((v & (2 * m - 1)) ^ m) - m

    assert np.array_equal(w[:, 0] & 4095, f["x0"]) and np.array_equal(w[:, 1] & 4095, f["y0"])
    assert np.array_equal((w[:, 0] >> 12) & 1023, f["dx1"]) and np.array_equal(sext(w[:, 1] >> 12, 10), f["dy1"])
    assert np.array_equal(np.stack([sext(w[:, 0] >> 22, 3), sext(w[:, 0] >> 25, 3)], axis=1), f["ddx"])
    assert np.array_equal(np.stack([sext(w[:, 1] >> 22, 3), sext(w[:, 1] >> 25, 3)], axis=1), f["ddy"])
    e = np.stack([sext(w[:, 0] >> 28, 2), sext(w[:, 0] >> 30, 2), sext(w[:, 1] >> 28, 2), sext(w[:, 1] >> 30, 2)], axis=1)
    assert np.array_equal(e, f["e"])
    # the product's decoder on words assembled here: x = 100, +5, +5 + 3, +8 - 4; y = 4095, -32, -32 - 1, -33 + 2; e = 1, -2, 0, -1; K = 5000
    one = np.array([100 | 5 << 12 | (3 & 7) << 22 | (-4 & 7) << 25 | (1 & 3) << 28 | (-2 & 3) << 30,
                    4095 | (-32 & 1023) << 12 | (-1 & 7) << 22 | (2 & 7) << 25 | (0 & 3) << 28 | (-1 & 3) << 30], np.uint32)
    back = np.zeros(12, np.int32)
    tap_lib.tap8_decode_words(one.ctypes.data, 5000, back.ctypes.data)
    y = [4095, 4063, 4030, 3999]
    assert back.tolist() == [100, 105, 113, 117] + y + [5000 - y[0] + 1, 5000 - y[1] - 2, 5000 - y[2], 5000 - y[3] - 1]


def test_both_forms_decode_to_the_same_twelve_numbers(tap_lib, limits):
    """Coordinates inside both formats (steps within the 12-byte entry's 7 / 6 bits, every step of x non-negative, y2 inside its
    12-bit base and 6-bit steps): the 12-byte decoder and the compact one, given K, return the same x, y and y2."""
    rng = np.random.default_rng(99)
    n = 300_000
    f = random_fields(rng, n, limits, dx_max=127, dy_lim=(-32, 31))
    f["K"] = f["y0"] + rng.integers(0, 4096, n)  # y2[0] = K - y[0] + e[0] near the 12-bit range
    coords = from_fields(**f)
    fit8, _, back8, fit12, back12 = run_many(tap_lib, coords, f["K"])
    assert fit8.all()
    both = fit8 & fit12
    assert both.sum() > n // 10, int(both.sum())
    assert np.array_equal(back8[both], coords[both])
    assert np.array_equal(back12[both], back8[both])


def test_stand_alone_walk_under_the_sanitizers(tmp_path):
    """The same header in a program of its own (tests/host_tap_table/tap8.cpp -DTAP8_MAIN), built with AddressSanitizer and UBSan:
    extremes of every field, 200 000 pseudo-random entries, and the encoder on values that do not fit."""
    exe = tmp_path / "tap8_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DTAP8_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-o", str(exe), str(HARNESS)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ", 0 bad" in r.stdout
