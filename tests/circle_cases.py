"""The smallest images at which each part of the image-circle fit can go wrong, shared by
tests/test_circle_host.py and tests/test_gpu_circle.py: one table of cases, one reference per case (tests/circle_ref.py), computed once.

A case is a base array, a slice of it (the view the fit reads: contiguous, pitched, or starting at an odd element), the parameters and,
for the discs with a known centre, the truth."""
from __future__ import annotations

import functools
from typing import Any, NamedTuple

import numpy as np

import circle_ref as R

WIDTHS = (1, 2, 4, 63, 64, 65, 127, 128, 129, 257)  # a step / a strip of 64 and their boundaries
HEIGHTS = (1, 2, 3, 4, 64, 65)


class Case(NamedTuple):
    base: np.ndarray
    view: tuple  # slices into base
    kw: dict
    truth: Any  # (cx, cy) or None

    @property
    def img(self) -> np.ndarray:
        return self.base[self.view]


FULL = (slice(None), slice(None))


def disc(h, w, cx, cy, r, *, cn=3, dtype=np.uint8, value=None, aa=True) -> np.ndarray:
    """a disc of `value` on black; anti-aliased: every pixel's value is its 4 x 4 sub-sample coverage of the disc"""
    top = np.iinfo(dtype).max
    value = int(top * 0.8) if value is None else value
    if aa:
        s = (np.arange(4) + 0.5) / 4 - 0.5
        yy = (np.arange(h)[:, None] + s[None, :]).reshape(-1)
        xx = (np.arange(w)[:, None] + s[None, :]).reshape(-1)
        inside = ((xx[None, :] - cx) ** 2 + (yy[:, None] - cy) ** 2 <= r * r).astype(np.float64)
        cov = inside.reshape(h, 4, w, 4).mean(axis=(1, 3))
    else:
        cov = ((np.arange(w)[None, :] - cx) ** 2 + (np.arange(h)[:, None] - cy) ** 2 <= r * r).astype(np.float64)
    a = np.floor(cov * value + 0.5).astype(dtype)
    return np.repeat(a[..., None], cn, axis=2)


def _speckled(h, w, seed, cn=3):
    """a disc where there is room for one, and lit pixels drawn at p = 0.35 around it: runs of every length at every position"""
    rng = np.random.default_rng(seed)
    a = disc(h, w, w / 2 - 0.3, h / 2 + 0.2, 0.38 * min(h, w), cn=cn, aa=False) if min(h, w) >= 4 else np.zeros((h, w, cn), np.uint8)
    a[rng.random((h, w)) < 0.35] = 90
    return a


def _lines(h, w, runs, axis):
    """a black image with lit runs [(line, start, length), ...] along rows (axis 0) or columns (axis 1)"""
    a = np.zeros((h, w, 3), np.uint8)
    for k, s, n in runs:
        if axis == 0:
            a[k, s:s + n] = 200
        else:
            a[s:s + n, k] = 200
    return a


@functools.lru_cache(maxsize=None)
def shared_cases() -> dict:
    c: dict[str, Case] = {}

    def add(name, base, view=FULL, truth=None, **kw):
        assert name not in c
        c[name] = Case(base, view, kw, truth)

    for i, w in enumerate(WIDTHS):
        for j, h in enumerate(HEIGHTS):
            add(f"size_{h}x{w}", _speckled(h, w, 100 * i + j), min_points=3)
    # a run that starts on lane 61 .. 63 of a step and crosses into the next one, from both ends; columns read 16 rows per batch and
    # 64 columns per strip
    for s in (61, 62, 63):
        add(f"row_cross_left_{s}", _lines(6, 200, [(1, s, 4), (2, 64 + s, 5), (3, s, 3), (3, 100, 4)], 0), min_points=3)
        add(f"row_cross_right_{s}", _lines(6, 200, [(1, 200 - s - 4, 4), (2, 200 - 64 - s - 5, 5), (4, 200 - s - 3, 3), (4, 20, 4)], 0), min_points=3)
        add(f"col_cross_top_{s}", _lines(200, 70, [(1, s, 4), (65, 64 + s, 5), (3, s, 3), (3, 100, 4)], 1), min_points=3)
        add(f"col_cross_bottom_{s}", _lines(200, 70, [(1, 200 - s - 4, 4), (66, 200 - 64 - s - 5, 5), (4, 200 - s - 3, 3), (4, 20, 4)], 1), min_points=3)
    for s in (13, 14, 15):
        add(f"col_cross_batch_{s}", _lines(40, 9, [(1, s, 4), (2, 16 + s, 6), (3, 40 - s - 4, 4)], 1), min_points=3)
    # runs of run - 1 (ignored) and of run, at the default and at other run lengths
    for run in (1, 2, 4, 7, 64):
        base = _lines(12, 300, [(1, 5, run - 1), (1, 5 + run + 2, run), (2, 40, run), (3, 290 - run, run - 1), (3, 200, run), (4, 10, 2 * run)], 0) if run > 1 \
            else _lines(12, 300, [(1, 7, 1), (2, 40, 1), (3, 200, 1), (4, 10, 2)], 0)
        add(f"run_{run}", base, run=run, min_points=3)
    # the rim on the frame's first / last two columns and rows
    for x in (0, 1, 98, 99):
        add(f"rim_col_{x}", _lines(20, 100, [(y, min(x, 96), 100 - min(x, 96)) for y in range(3, 17)] if x < 2 else
                                   [(y, 0, x + 1) for y in range(3, 17)], 0), min_points=3)
    for y in (0, 1, 38, 39):
        add(f"rim_row_{y}", _lines(40, 30, [(x, min(y, 36), 40 - min(y, 36)) for x in range(3, 27)] if y < 2 else
                                   [(x, 0, y + 1) for x in range(3, 27)], 1), min_points=3)
    # discs clipped by the frame on one, two, three and four sides (96 x 80 frames)
    add("clip_1", disc(80, 96, 30.3, 40.2, 34), truth=(30.3, 40.2))
    add("clip_2", disc(80, 96, 30.3, 28.6, 34), truth=(30.3, 28.6))
    add("clip_3", disc(80, 96, 44.7, 36.4, 46), truth=(44.7, 36.4))
    add("clip_4", disc(80, 96, 47.6, 40.3, 50), truth=(47.6, 40.3))
    add("all_black", np.zeros((33, 70, 3), np.uint8))
    add("all_lit", np.full((33, 70, 3), 255, np.uint8))
    one = np.zeros((33, 70, 3), np.uint8)
    one[17, 40] = 255
    add("one_lit_pixel", one)
    add("one_lit_pixel_run_1", one, run=1, min_points=3)
    # a dark wedge on the rim and hot pixels in the border
    wedge = disc(160, 200, 101.3, 77.6, 60)
    wedge[70:86, 30:70] = 0
    add("wedge", wedge, truth=(101.3, 77.6))
    hot = disc(160, 200, 101.3, 77.6, 60)
    rng = np.random.default_rng(7)
    for y, x in zip(rng.integers(0, 160, 300), rng.integers(0, 200, 300)):
        if (x - 101.3) ** 2 + (y - 77.6) ** 2 > 66 ** 2:
            hot[y, x] = 255
    add("hot_pixels", hot, truth=(101.3, 77.6))
    # thresholds
    add("threshold_0", disc(40, 50, 25, 20, 12), threshold=0)
    add("threshold_255", disc(40, 50, 25.4, 20.3, 14, value=255), threshold=255)
    add("threshold_255_alpha", disc(40, 50, 25.4, 20.3, 14, value=255, cn=4), threshold=255)
    add("threshold_65535_u8", disc(40, 50, 25, 20, 12, value=255), threshold=65535)
    add("threshold_65535_u16", disc(40, 50, 25.4, 20.3, 14, dtype=np.uint16, value=65535), threshold=65535)
    # channel counts and 16-bit pixels: only the SUM of the channels decides -- one bright channel lights a pixel, alpha counts
    for cn in (1, 3, 4):
        for dt in (np.uint8, np.uint16):
            a = disc(70, 90, 44.6, 33.3, 28, cn=cn, dtype=dt)
            if cn > 1:
                a[..., 0] = 0  # the mean over the channels is still above the threshold
            add(f"cn{cn}_{np.dtype(dt).name}", a, truth=(44.6, 33.3))
    dim = np.zeros((70, 90, 4), np.uint8)
    dim[..., 3] = disc(70, 90, 44.6, 33.3, 28, cn=1, value=40)[..., 0]  # alpha alone: 40 / 4 = 10 >= threshold
    add("alpha_only", dim, truth=(44.6, 33.3))
    dim39 = dim.copy()
    dim39[dim39 == 40] = 39  # 39 < 4 * 10
    add("alpha_just_below", dim39)
    # views: a half of a side-by-side frame (pitched), views that start at an odd element
    for dt in (np.uint8, np.uint16):
        n = np.dtype(dt).name
        sbs = np.concatenate([disc(70, 90, 40.2, 36.7, 30, dtype=dt), disc(70, 90, 50.8, 30.1, 27, dtype=dt)], axis=1)
        add(f"view_left_half_{n}", sbs, (slice(None), slice(0, 90)), truth=(40.2, 36.7))
        add(f"view_right_half_{n}", sbs, (slice(None), slice(90, 180)), truth=(50.8, 30.1))
        add(f"view_odd_offset_{n}", sbs, (slice(1, 69), slice(91, 180)), truth=(49.8, 29.1))
        g = np.concatenate([disc(70, 91, 40.2, 36.7, 30, dtype=dt, cn=1)] * 2, axis=1)
        add(f"view_odd_offset_gray_{n}", g, (slice(None), slice(91, 182)), truth=(40.2, 36.7))
    # anti-aliased discs at fractional centres
    for k, (cx, cy, r) in enumerate([(64.0, 64.5, 50.0), (70.25, 58.75, 41.3), (61.5, 66.125, 55.8), (130.37, 99.81, 90.4)]):
        h, w = (129, 128) if k < 3 else (200, 257)
        add(f"aa_disc_{k}", disc(h, w, cx, cy, r), truth=(cx, cy))
    return c


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(eight doubles, (n, 3) rim points) of a case by the restatement; shared, never modified"""
    case = shared_cases()[name]
    out, rim = R.fit(case.img, **case.kw)
    out.setflags(write=False)
    rim.setflags(write=False)
    return out, rim
