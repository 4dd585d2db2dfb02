"""Adversarial cases for the 16-bit / float32 remap (k_remap_wide behind v1c_remap_lut_ex; sample_wide on the host), shared by the
host half (tests/test_wide_host.py) and the GPU half (tests/test_gpu_wide_lut.py).  Not a test module.  Seeded and deterministic.

``cases(dtype, interp)`` walks border x cn and draws everything else: sources of 1 x 1 ... 40 x 33 px, output widths either side of
the lane's 4 pixels and of the workgroup's 256-pixel column, output heights around the 4-row workgroup, the three map kinds of
tools/fuzz.py::lut_case sprinkled with the values the fixed-point conversion treats specially, a map pitch pad, a random prefilled
destination (BORDER_TRANSPARENT keeps it) and a view description for source and destination: contiguous, pitched behind a dword-aligned
offset, or pitched behind an odd element offset -- which leaves a uint16 destination 2-byte aligned only, as an odd pitch in elements
does for every second row.  A third of the float32 sources hold denormals, values next to FLT_MAX, signed zeros, infinities and NaN.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any

import numpy as np

DTYPES = (np.uint16, np.float32)
INTERPS = (0, 1, 2, 3, 4)
BORDERS = (0, 1, 2, 3, 4, 5)
CNS = (1, 3, 4)
# (the first five: the values the host sampler was checked with; the rest: tests/test_gpu_wide.py's BVS)
BORDER_VALUES = [70000, -3, 2.5, (1.5, 0.25, -3, 2.5), (1e-40, 3e38, -1, 2), 1.5, 0.25, (70000, -3, 2.5)]
SRC_KINDS = ("1x1", "1xN", "Nx1", "2x2", "7x9", "40x33")
OUT_WIDTHS = (1, 3, 4, 5, 255, 256, 257, 260, 515)
OUT_HEIGHTS = (1, 3, 4, 5, 9)
MAP_KINDS = ("affine+noise", "around", "grid-ties")
MAP_PADS = (0, 4, 8)
VIEWS = ("contiguous", "pitched-dword", "pitched-odd")
EXTREME_PIXELS = np.array([1e-45, -1e-45, 1e-39, 1.1754943508222875e-38, 3.4e38, -3.4e38, 0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
ROUNDS = 4  # cases per (dtype, interp, border, cn)


@dataclass
class View:
    """where an (h, w, cn) image lies inside a flat buffer of its element type: element offset and row pitch in elements"""
    kind: str
    offset: int
    pitch: int
    size: int  # elements of the buffer


@dataclass
class Case:
    dtype: Any
    interp: int
    border: int
    cn: int
    bv: Any
    src: np.ndarray      # (hs, ws, cn), contiguous
    xm: np.ndarray       # (ho, wo) float32
    ym: np.ndarray
    map_kind: str
    map_pad: int         # floats behind every map row on the device
    fill: np.ndarray     # (ho, wo, cn): what the destination holds before the call
    src_kind: str
    src_view: View
    dst_view: View
    extremes: bool
    seed: tuple

    def __str__(self) -> str:
        ho, wo = self.xm.shape
        return (f"{np.dtype(self.dtype).name} interp={self.interp} border={self.border} cn={self.cn} bv={self.bv!r} src={self.src.shape[1]}x"
                f"{self.src.shape[0]} ({self.src_kind}) out={wo}x{ho} maps={self.map_kind} map_pad={self.map_pad} src_view={self.src_view} "
                f"dst_view={self.dst_view} extremes={self.extremes} seed={self.seed}")


def special_values(hs: int, ws: int) -> np.ndarray:
    """tools/fuzz.py::lut_case's list: what cv2's fixed-point conversion of a map coordinate treats specially"""
    return np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, -3e9, 2.0 ** 26, -(2.0 ** 26), 67108863.0, 32767.0, 32767.5, 32768.0, -32768.0,
                     -32768.5, -32769.0, -0.5, -1.0, 0.0, -0.0, ws - 1.0, ws - 0.5, float(ws), hs - 1.0, float(hs), 1e-30, -1e-30], np.float32)


def draw_maps(rng, kind: int, ho: int, wo: int, hs: int, ws: int):
    """the three kinds of tools/fuzz.py::lut_case, each sprinkled with ``special_values``"""
    jj, ii = np.mgrid[:ho, :wo].astype(np.float64)
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
    special = special_values(hs, ws)
    for m in (xm, ym):
        k = int(rng.integers(0, max(2, m.size // 20)))
        m.reshape(-1)[rng.integers(0, m.size, k)] = rng.choice(special, k)
    return xm, ym


def draw_pixels(rng, dtype, shape, extremes: bool = False) -> np.ndarray:
    if np.dtype(dtype) == np.uint16:
        a = rng.integers(0, 65536, shape).astype(np.uint16)
        a[rng.random(shape) < 0.05] = 65535
        return a
    a = rng.normal(0.5, 2.0, shape).astype(np.float32)
    if extremes:
        m = rng.random(shape) < 0.3
        a[m] = rng.choice(EXTREME_PIXELS, int(m.sum()))
    return a


def draw_view(rng, kind: str, h: int, w: int, cn: int, dtype) -> View:
    row = w * cn
    if kind == "contiguous":
        return View(kind, 0, row, h * row)
    per_dword = 4 // np.dtype(dtype).itemsize
    if kind == "pitched-dword":  # offset and pitch whole dwords
        offset = per_dword * int(rng.integers(0, 5))
        pitch = row + int(rng.integers(0, 9))
        pitch += -pitch % per_dword
    else:  # an odd element offset; the pitch odd or even
        offset = 2 * int(rng.integers(0, 4)) + 1
        pitch = row + int(rng.integers(0, 9))
    return View(kind, offset, pitch, offset + h * pitch + int(rng.integers(0, 5)))


def place(view: View, img: np.ndarray, rng=None) -> np.ndarray:
    """the flat buffer of ``view`` with ``img`` inside it; the elements around the image are random (seeded by the view) and finite"""
    pad = draw_pixels(np.random.default_rng([view.offset, view.pitch, view.size]) if rng is None else rng, img.dtype, (view.size,))
    window(view, pad, img.shape)[...] = img
    return pad


def window(view: View, buf: np.ndarray, shape) -> np.ndarray:
    """the (h, w, cn) image inside the flat buffer, as a strided view of it"""
    h, w, cn = shape
    isz = buf.dtype.itemsize
    return np.lib.stride_tricks.as_strided(buf[view.offset:], (h, w, cn), (view.pitch * isz, cn * isz, isz))


def _src_size(rng, kind: str):
    n = int(rng.integers(2, 40))
    return {"1x1": (1, 1), "1xN": (1, n), "Nx1": (n, 1), "2x2": (2, 2), "7x9": (7, 9), "40x33": (40, 33)}[kind]  # (h, w)


def cases(dtype, interp: int):
    """the cases of one pixel type and interpolation: ROUNDS per border x cn; widths, heights and destination views cycle so that every
    (dtype, interp) sees all of them, the rest is drawn"""
    di = DTYPES.index(dtype)
    i = 0
    for border in BORDERS:
        for cn in CNS:
            for rnd in range(ROUNDS):
                seed = (77, di, interp, border, cn, rnd)
                rng = np.random.default_rng(seed)
                wo = OUT_WIDTHS[(i + interp) % len(OUT_WIDTHS)]
                ho = OUT_HEIGHTS[(i // 2 + di) % len(OUT_HEIGHTS)]
                dst_kind = VIEWS[(rnd + CNS.index(cn) + border) % 3]  # (every border x cn sees the three kinds)
                src_kind = SRC_KINDS[int(rng.integers(len(SRC_KINDS)))]
                hs, ws = _src_size(rng, src_kind)
                extremes = np.dtype(dtype) == np.float32 and i % 3 == (interp % 3)
                src = draw_pixels(rng, dtype, (hs, ws, cn), extremes)
                mk = int(rng.integers(3))
                xm, ym = draw_maps(rng, mk, ho, wo, hs, ws)
                fill = draw_pixels(rng, dtype, (ho, wo, cn))
                yield Case(dtype=dtype, interp=interp, border=border, cn=cn, bv=BORDER_VALUES[int(rng.integers(len(BORDER_VALUES)))],
                           src=src, xm=xm, ym=ym, map_kind=MAP_KINDS[mk], map_pad=MAP_PADS[int(rng.integers(3))], fill=fill,
                           src_kind=src_kind, src_view=draw_view(rng, VIEWS[int(rng.integers(3))], hs, ws, cn, dtype),
                           dst_view=draw_view(rng, dst_kind, ho, wo, cn, dtype), extremes=bool(extremes), seed=seed)
                i += 1


def all_cases():
    for dtype in DTYPES:
        for interp in INTERPS:
            yield from cases(dtype, interp)


def same(got: np.ndarray, want: np.ndarray) -> bool:
    """byte for byte; float32: equal, with NaN <=> NaN"""
    if got.dtype == np.uint16:
        return got.tobytes() == want.tobytes()
    return np.array_equal(got, want, equal_nan=True)


def ndiff(got: np.ndarray, want: np.ndarray) -> int:
    g, w = got.astype(np.float64), want.astype(np.float64)
    return int((~((g == w) | (np.isnan(g) & np.isnan(w)))).sum())
