"""The smallest pairs of eyes at which each part of the colour match can go wrong, shared by
tests/test_colormatch_host.py and tests/test_gpu_colormatch.py: one table of cases, one reference per case (tests/colormatch_ref.py),
computed once.

A case is ONE base buffer of bytes, the two eyes as views into it (offset and row pitch in bytes: contiguous, padded, the halves of a
side-by-side frame, rows that start at an odd byte), the parameters, and whether the target eye is rewritten in place."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import colormatch_ref as R

FILL = 0xA5  # what the base holds outside the eyes: a stray store shows


class Case(NamedTuple):
    base: np.ndarray  # 1-D uint8
    shape: tuple      # (h, w, cn)
    left: tuple       # (offset, pitch) in bytes
    right: tuple
    kw: dict
    inplace: bool

    def view(self, which: str, base: np.ndarray | None = None) -> np.ndarray:
        off, pitch = self.left if which == "left" else self.right
        h, w, cn = self.shape
        b = self.base if base is None else base
        return np.lib.stride_tricks.as_strided(b[off:], (h, w, cn), (pitch, cn, 1))

    @property
    def target(self) -> str:
        return "right" if self.kw.get("reference", "left") == "left" else "left"


def disc_mask(h, w, cx=None, cy=None, r=None):
    cx, cy = (w - 1) / 2 if cx is None else cx, (h - 1) / 2 if cy is None else cy
    r = 0.45 * min(h, w) if r is None else r
    return (np.arange(w)[None, :] - cx) ** 2 + (np.arange(h)[:, None] - cy) ** 2 <= r * r


def noise_disc(h, w, cn, seed, lo=10, hi=180, **disc):
    """uniform noise in [lo, hi] inside a disc, black around it; a fourth channel is noise everywhere"""
    rng = np.random.default_rng(seed)
    a = rng.integers(lo, hi + 1, (h, w, cn), dtype=np.uint8)
    a[~disc_mask(h, w, **disc), : (1 if cn == 1 else 3)] = 0
    return a


def brighter(a):
    """L + (L >> 2) on the colour channels: strictly increasing on [0, 204], so a match can undo it exactly"""
    b = a.copy()
    nc = 1 if a.shape[2] == 1 else 3
    b[..., :nc] = a[..., :nc] + (a[..., :nc] >> 2)
    return b


def carve(L, R_, *, pad_l=0, pad_r=0, off=0, sbs=False, pad=0, kw=None, inplace=True) -> Case:
    """the two eyes laid into one buffer: each with its own padded pitch behind `off` bytes, or as the halves of a side-by-side frame
    whose rows are 2 w cn + pad bytes"""
    h, w, cn = L.shape
    row = w * cn
    if sbs:
        pitch = 2 * row + pad
        left, right = (off, pitch), (off + row, pitch)
        size = off + h * pitch
    else:
        pl, pr = row + pad_l, row + pad_r
        o2 = off + h * pl + 7  # (the second eye starts 7 bytes further than it has to: another residue modulo 16)
        left, right = (off, pl), (o2, pr)
        size = o2 + h * pr
    base = np.full(size + 3, FILL, np.uint8)
    c = Case(base, (h, w, cn), left, right, dict(kw or {}), inplace)
    c.view("left")[...] = L
    c.view("right")[...] = R_
    base.setflags(write=False)
    return c


def recovery_pair(seed=0, h=67, w=131, cn=3):
    """the issue's exact-recovery pair: a disc of uniform noise in [10, 180] on black and R = L + (L >> 2)"""
    L = noise_disc(h, w, cn, seed)
    return L, brighter(L)


def gain_pair(seed=1, h=67, w=131):
    L = noise_disc(h, w, 3, seed)
    return L, np.minimum(255, (5 * L.astype(np.int32) + 2) // 4).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def shared_cases() -> dict:
    few = dict(min_pixels=16)
    cases = {}
    # rows of 3, 15 and 63 bytes (all head and tail, or one 16-byte body), one row, one column
    for h, w in ((9, 1), (9, 5), (9, 21), (1, 131), (40, 1)):
        L = noise_disc(h, w, 3, 10 + w, r=1e9)
        cases[f"small_{h}x{w}"] = carve(L, brighter(L), kw=dict(min_pixels=1))
        cases[f"small_{h}x{w}_gain_out"] = carve(L, brighter(L), off=5, kw=dict(min_pixels=1, mode="gain"), inplace=False)
    L, Rr = recovery_pair()
    cases["recovery"] = carve(L, Rr, kw=few)
    cases["recovery_right_reference"] = carve(Rr, L, kw=dict(few, reference="right"))
    cases["recovery_out_of_place"] = carve(L, Rr, kw=few, inplace=False)
    cases["gain"] = carve(*gain_pair(), kw=dict(few, mode="gain"))
    cases["gain_right_reference"] = carve(*gain_pair()[::-1], kw=dict(few, mode="gain", reference="right"), inplace=False)
    cases["padded"] = carve(L, Rr, pad_l=13, pad_r=32, off=3, kw=few)
    for cn in (1, 4):
        a = noise_disc(67, 131, cn, 20 + cn)
        cases[f"cn{cn}"] = carve(a, brighter(a), kw=few)
        cases[f"cn{cn}_gain_sbs"] = carve(a, brighter(a), sbs=True, pad=5, off=1, kw=dict(few, mode="gain"), inplace=cn == 4)
    # the halves of an odd-width side-by-side frame: the right eye's rows start at an odd byte
    cases["sbs_odd"] = carve(L, Rr, sbs=True, kw=few)
    cases["sbs_odd_right_reference"] = carve(L, Rr, sbs=True, off=2, pad=3, kw=dict(few, reference="right"))
    cases["sbs_odd_gain"] = carve(L, Rr, sbs=True, kw=dict(few, mode="gain"))
    # contents
    flat_l, flat_r = np.full((67, 131, 3), 100, np.uint8), np.full((67, 131, 3), 140, np.uint8)
    cases["flat"] = carve(flat_l, flat_r, kw=few)
    cases["flat_gain"] = carve(flat_l, flat_r, kw=dict(few, mode="gain"))
    g = np.broadcast_to((np.arange(131) * 255 // 130).astype(np.uint8)[None, :, None], (67, 131, 3)).copy()
    cases["gradient"] = carve(g, (g // 2 + 20).astype(np.uint8), kw=few)
    # the eyes' black surrounds differ: a pixel lit in one eye and black in the other must not count
    a, b = noise_disc(67, 131, 3, 30, cx=50, cy=30, r=28), brighter(noise_disc(67, 131, 3, 30, cx=80, cy=36, r=28))
    cases["surrounds_differ"] = carve(a, b, kw=few)
    cases["surrounds_differ_gain"] = carve(a, b, kw=dict(few, mode="gain"))
    # statuses
    cases["status1_default_min_pixels"] = carve(L[:20, :40].copy(), Rr[:20, :40].copy())
    black = np.zeros((20, 40, 3), np.uint8)
    cases["status2_black_gain"] = carve(black, black.copy(), kw=dict(mode="gain", lo=0, min_pixels=1))
    cases["black_histogram_lo0"] = carve(black, black.copy(), kw=dict(lo=0, min_pixels=1))
    cases["empty_mask_min_pixels_0"] = carve(black, black.copy(), kw=dict(min_pixels=0))
    # parameters off the defaults
    dark = noise_disc(67, 131, 3, 40, lo=10, hi=60)
    cases["max_shift_clamps"] = carve((dark + 120).astype(np.uint8) * (dark > 0), dark, kw=dict(few, max_shift=20))
    clip = L.copy()
    clip[20:40, 40:90] = 255
    cases["hi_keeps_clipped_out"] = carve(clip, brighter(clip), kw=few)
    cases["hi_255_counts_clipped"] = carve(clip, brighter(clip), kw=dict(few, hi=255))
    cases["lo_hi_narrow"] = carve(L, Rr, kw=dict(few, lo=60, hi=120, max_shift=255))
    cases["gain_clamped_low"] = carve(np.full((20, 40, 3), 12, np.uint8), np.full((20, 40, 3), 200, np.uint8), kw=dict(few, mode="gain"))
    cases["gain_clamped_high"] = carve(np.full((20, 40, 3), 200, np.uint8), np.full((20, 40, 3), 12, np.uint8), kw=dict(few, mode="gain"))
    return cases


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(result, luts, report, histograms) of the restatement; the result is the rewritten target eye"""
    return reference_of(shared_cases()[name])


def reference_of(case: Case):
    p = dict(R.DEFAULTS, **case.kw)
    luts, report, hist = R.luts(case.view("left"), case.view("right"), **p)
    return R.apply_luts(case.view(case.target), luts), luts, report, hist


def expected_base(case: Case, result: np.ndarray) -> np.ndarray:
    """the base buffer after an in-place match: the target eye's bytes are the result's, every other byte is as it was"""
    b = case.base.copy()
    if case.inplace:
        case.view(case.target, b)[...] = result
    return b
