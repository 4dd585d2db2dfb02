"""The smallest images at which each part of the vignetting correction can go wrong, shared by
tests/test_vignette_host.py and tests/test_gpu_vignette.py: one table of cases, one reference per case (tests/vignette_ref.py),
computed once.

A case is ONE base buffer of bytes, the image as a view into it (offset and row pitch in bytes: contiguous, padded, the right half of
a side-by-side frame, rows that start at an odd byte), the circle, the model, the ring parameters, and whether the image is rewritten
in place."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import vignette_ref as R

FILL = 0xA5  # what the base holds outside the image: a stray store shows


class Case(NamedTuple):
    base: np.ndarray  # 1-D uint8
    shape: tuple      # (h, w, cn)
    dtype: type       # np.uint8 / np.uint16
    off: int          # bytes
    pitch: int        # bytes
    center: tuple     # (cx, cy), integers
    radius: float
    coefs: tuple      # ((k1, k2, k3) x BGR, gamma)
    rings: int
    lo: int
    hi: int
    inplace: bool

    def view(self, base: np.ndarray | None = None) -> np.ndarray:
        h, w, cn = self.shape
        es = np.dtype(self.dtype).itemsize
        b = self.base if base is None else base
        return np.ndarray((h, w, cn), self.dtype, buffer=b, offset=self.off, strides=(self.pitch, cn * es, es))

    def vignette(self):
        from vr180_convert_amd.vignette import Vignette

        (b, g, r), gamma = self.coefs
        return Vignette(gamma=gamma, blue=b, green=g, red=r)


STRONG = (((-0.35, -0.2, 0.05), (-0.3, -0.25, 0.04), (-0.4, -0.1, -0.05)), 1.0)   # about one and a half stops at the rim
ENCODED = (((-0.3, -0.2, 0.0),) * 3, 2.2)
IDENTITY = (((0.0, 0.0, 0.0),) * 3, 1.0)


def noise(h, w, cn, dtype, seed, lo=None, hi=None):
    rng = np.random.default_rng(seed)
    top = 255 if dtype == np.uint8 else 65535
    return rng.integers(top // 25 if lo is None else lo, (top * 3 // 4 if hi is None else hi) + 1, (h, w, cn)).astype(dtype)


def carve(img, *, off=0, pad=0, sbs=False, center=None, radius=None, coefs=STRONG, rings=16, lo=None, hi=None, inplace=False) -> Case:
    """the image laid into a buffer behind `off` bytes with rows of w cn es + pad bytes, or as the RIGHT half of a side-by-side frame of
    twice its width (+ pad)"""
    h, w, cn = img.shape
    es = img.dtype.itemsize
    row = w * cn * es
    pitch = (2 * row if sbs else row) + pad
    off = off + (row if sbs else 0)
    assert off % es == 0 and pitch % es == 0
    size = off + (h - 1) * pitch + row
    base = np.full(size + (pitch - row if sbs else 0) + 2 * es, FILL, np.uint8)
    top = 255 if img.dtype == np.uint8 else 65535
    c = Case(base, (h, w, cn), img.dtype.type, off, pitch, (w // 2, h // 2) if center is None else center,
             0.5 * max(h, w) if radius is None else radius, coefs, rings, top // 25 if lo is None else lo, top - 1 if hi is None else hi, inplace)
    c.view()[...] = img
    base.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def shared_cases() -> dict:
    cases = {}
    # head / segment / tail: rows of 1, 15, 16, 17 pixels and three rows of 45
    for h, w in ((1, 1), (1, 15), (1, 16), (1, 17), (3, 45)):
        for dt in (np.uint8, np.uint16):
            cases[f"small_{h}x{w}_{np.dtype(dt).name}"] = carve(noise(h, w, 3, dt, 10 + w), radius=max(2.0, w / 2), off=np.dtype(dt).itemsize)
    for cn in (1, 3, 4):
        for dt in (np.uint8, np.uint16):
            cases[f"cn{cn}_{np.dtype(dt).name}"] = carve(noise(37, 83, cn, dt, 20 + cn), radius=44.0, inplace=cn == 4)
    # the right half of a 91-wide side-by-side view: rows start at an odd byte (uint8) / off every 16-byte boundary (uint16)
    for dt in (np.uint8, np.uint16):
        n = np.dtype(dt).name
        cases[f"sbs_odd_{n}"] = carve(noise(37, 91, 3, dt, 31), sbs=True, radius=40.5, center=(44, 19))
        cases[f"sbs_odd_inplace_{n}"] = carve(noise(37, 91, 3, dt, 32), sbs=True, pad=np.dtype(dt).itemsize, off=np.dtype(dt).itemsize,
                                               radius=40.5, inplace=True)
        cases[f"pitch_gap_{n}"] = carve(noise(37, 83, 3, dt, 33), pad=26, off=6, radius=44.0, coefs=ENCODED)
        cases[f"inplace_{n}"] = carve(noise(37, 83, 3, dt, 34), radius=44.0, inplace=True)
        # a centre outside the frame, on either side
        cases[f"center_outside_{n}"] = carve(noise(37, 83, 3, dt, 35), center=(-60, 50), radius=150.0)
        cases[f"center_beyond_{n}"] = carve(noise(37, 83, 3, dt, 36), center=(160, -30), radius=100.0, rings=64)
        # a radius of 2: rings and table positions far coarser than pixels, and the hold of the last interval
        cases[f"radius_2_{n}"] = carve(noise(37, 83, 3, dt, 37), radius=2.0)
        cases[f"rings_1024_{n}"] = carve(noise(37, 83, 3, dt, 38), radius=44.0, rings=1024)
        # a flat frame (one run per thread and ring) and the identity model
        cases[f"flat_{n}"] = carve(np.full((37, 83, 3), 100 if dt == np.uint8 else 30000, dt), radius=44.0)
        cases[f"identity_{n}"] = carve(noise(37, 83, 3, dt, 39), radius=44.0, coefs=IDENTITY)
        # the mask leaves nothing
        cases[f"masked_out_{n}"] = carve(noise(37, 83, 3, dt, 40, lo=0, hi=5), radius=44.0)
    # saturation: bright pixels under a gain of almost 4
    cases["saturates_uint8"] = carve(noise(37, 83, 3, np.uint8, 41, lo=100, hi=255), radius=44.0, coefs=(((-0.9, 0.0, 0.0),) * 3, 1.0), hi=255)
    cases["saturates_uint16"] = carve(noise(37, 83, 3, np.uint16, 42, lo=30000, hi=65535), radius=44.0, coefs=(((-0.9, 0.0, 0.0),) * 3, 1.0), hi=65535)
    return cases


def geometry(case: Case):
    """(cx, cy, scale, shift, R2) as the package's host code gives them"""
    from vr180_convert_amd import vignette as V

    h, w, _ = case.shape
    g = V.geometry(h, w, case.center, case.radius)
    return g.cx, g.cy, g.scale, g.shift, V.ring_r2(case.radius)


def tables(case: Case) -> np.ndarray:
    from vr180_convert_amd import vignette as V

    return V.gain_tables(case.vignette())


def reference_of(case: Case):
    """(result, ring record) of the restatement"""
    cx, cy, scale, shift, R2 = geometry(case)
    img = case.view()
    return R.apply(img, tables(case), cx, cy, scale, shift), R.rings(img, cx, cy, R2, case.rings, case.lo, case.hi)


@functools.lru_cache(maxsize=None)
def reference(name: str):
    return reference_of(shared_cases()[name])


def expected_base(case: Case, result: np.ndarray) -> np.ndarray:
    """the base buffer after an in-place pass: the image's bytes are the result's, every other byte is as it was"""
    b = case.base.copy()
    if case.inplace:
        case.view(b)[...] = result
    return b


# ---- the round trip's flat field -------------------------------------------------------------------------------------------------------
def flat_field(v, h, w, center, radius, level, dtype, seed, sigma):
    """round(A / g(rho)) under the model `v`, plus Gaussian sensor noise of `sigma` levels, black outside the circle"""
    rng = np.random.default_rng(seed)
    r2 = R.r2_of(h, w, *center).astype(np.float64) / (radius * radius)
    img = level / v.gain(r2)  # (3, h, w)
    img = np.moveaxis(img, 0, 2) + rng.normal(0.0, sigma, (h, w, 3))
    top = 255 if dtype == np.uint8 else 65535
    out = np.clip(np.floor(img + 0.5), 0, top).astype(dtype)
    out[r2 >= 1.0] = 0
    return out
