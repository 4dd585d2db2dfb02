"""NumPy restatement of the image-circle fit's contract (v1c_fit_circle*): lit pixels, rim points, the integer
moment sums, the float64 solve as one written-out sequence of operations, the trimmed refits with their exact selection test, the
result.  Written from the contract, not from the kernels: whole-array operations where the device walks in steps of 64."""
from __future__ import annotations

import math

import numpy as np

DEFAULTS = {"threshold": 10, "run": 4, "rounds": 4, "min_points": 8, "tol16": (128, 48, 24, 24)}


def lit_mask(img: np.ndarray, threshold: int) -> np.ndarray:
    """(H, W) bool: sum of the channels >= threshold * cn, every channel counted"""
    a = img if img.ndim == 3 else img[..., None]
    if a.dtype not in (np.uint8, np.uint16):
        raise TypeError(f"uint8 or uint16 images only, not {a.dtype}")
    return a.astype(np.int64).sum(axis=2) >= int(threshold) * a.shape[2]


def _first_run(line: np.ndarray, run: int) -> int:
    """index of the first pixel of the first run of at least `run` lit pixels of a 1-D bool line, -1 without one"""
    n = len(line)
    if n < run:
        return -1
    c = np.concatenate([[0], np.cumsum(line.astype(np.int64))])
    full = np.nonzero(c[run:] - c[:-run] == run)[0]
    return int(full[0]) if len(full) else -1


def rim_points(lit: np.ndarray, run: int) -> list[tuple[int, int]]:
    """the rim points in order: per row (left, right), then per column (top, bottom); points on the frame's own edge dropped"""
    h, w = lit.shape
    pts = []
    for y in range(h):
        a = _first_run(lit[y], run)
        if a < 0:
            continue
        b = w - 1 - _first_run(lit[y, ::-1], run)
        pts += [(x, y) for x in (a, b) if 0 < x < w - 1]
    for x in range(w):
        a = _first_run(lit[:, x], run)
        if a < 0:
            continue
        b = h - 1 - _first_run(lit[::-1, x], run)
        pts += [(x, y) for y in (a, b) if 0 < y < h - 1]
    return pts


def moment_sums(x: np.ndarray, y: np.ndarray) -> list[int]:
    """N, Sx, Sy, Sxx, Sxy, Syy, Sxz, Syz, Sz with z = x^2 + y^2, as Python integers"""
    x, y = x.astype(np.int64), y.astype(np.int64)
    z = x * x + y * y
    return [int(v) for v in (len(x), x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum(), (x * z).sum(), (y * z).sum(), z.sum())]


def solve(s: list[int], h: int, w: int) -> tuple[float, float, float, int]:
    """(cx, cy, r, status) relative to (w // 2, h // 2); every operation a float64 one, in this order"""
    f = np.float64
    n = f(s[0])
    if not n > 0.0:
        return 0.0, 0.0, 0.0, 2
    sx, sy, sxx, sxy, syy, sxz, syz, sz = (f(v) for v in s[1:])
    with np.errstate(all="ignore"):
        mx, my = sx / n, sy / n
        suu, suv, svv = sxx - sx * mx, sxy - sx * my, syy - sy * my
        suz, svz = sxz - sz * mx, syz - sz * my
        det = suu * svv - suv * suv
        if not det > f(1e-12) * (suu * svv):
            return 0.0, 0.0, 0.0, 2
        cx = (suz * svv - svz * suv) / (f(2.0) * det)
        cy = (svz * suu - suz * suv) / (f(2.0) * det)
        r2 = ((cx * cx + cy * cy) + sz / n) - (f(2.0) * cx * mx + f(2.0) * cy * my)
        lim = f(max(h, w))
        if not r2 > 0.0:
            return 0.0, 0.0, 0.0, 3
        r = np.sqrt(r2)
        if not r <= 4.0 * lim or not abs(cx) <= 8.0 * lim or not abs(cy) <= 8.0 * lim:
            return 0.0, 0.0, 0.0, 3
    return float(cx), float(cy), float(r), 0


def q16(v: float) -> int:
    return int(math.floor(np.float64(v) * np.float64(16.0) + np.float64(0.5)))


def dist2_16(x: np.ndarray, y: np.ndarray, cx16: int, cy16: int) -> np.ndarray:
    dx, dy = 16 * x.astype(np.int64) - cx16, 16 * y.astype(np.int64) - cy16
    return dx * dx + dy * dy


def fit_points(pts, h: int, w: int, *, rounds: int, min_points: int, tol16) -> tuple[np.ndarray, np.ndarray]:
    """the eight doubles and the selection flag of every point"""
    p = np.asarray(pts, np.int64).reshape(-1, 2)
    x, y = p[:, 0] - w // 2, p[:, 1] - h // 2
    sel = np.ones(len(p), bool)
    n_rim = n_used = len(p)

    def failed(status):
        return np.array([0, 0, 0, status, n_rim, n_used, 0, 0], np.float64), sel

    cx = cy = r = 0.0
    for k in range(-1, rounds):
        if k >= 0:
            d2 = dist2_16(x, y, q16(cx), q16(cy))
            r16, t16 = q16(r), int(tol16[k])
            hi, lo = r16 + t16, r16 - t16
            sel = (d2 <= hi * hi) & ((d2 >= lo * lo) if lo > 0 else True)
            sel = np.broadcast_to(sel, x.shape).copy()
        n_used = int(sel.sum())
        if n_used < min_points:
            return failed(1)
        cx, cy, r, status = solve(moment_sums(x[sel], y[sel]), h, w)
        if status:
            return failed(status)
    cx16, cy16, r16 = q16(cx), q16(cy), q16(r)
    e = np.array([math.isqrt(int(v)) for v in dist2_16(x[sel], y[sel], cx16, cy16)], np.int64) - r16
    rms = float(np.sqrt(np.float64(int((e * e).sum())) / np.float64(n_used)) / np.float64(16.0))
    return np.array([np.float64(w // 2) + np.float64(cx), np.float64(h // 2) + np.float64(cy), r, 0, n_rim, n_used, rms, 0], np.float64), sel


def fit(img: np.ndarray, *, threshold=None, run=None, rounds=None, min_points=None, tol16=None):
    """(eight doubles, (n, 3) int32 rim points (x, y, selected)) of an (H, W[, C]) uint8 / uint16 image"""
    d = DEFAULTS
    threshold = d["threshold"] if threshold is None else threshold
    run = d["run"] if run is None else run
    tol16 = d["tol16"] if tol16 is None else tol16
    rounds = len(tol16) if rounds is None else rounds  # (one refit per tolerance given)
    min_points = d["min_points"] if min_points is None else min_points
    lit = lit_mask(img, threshold)
    h, w = lit.shape
    pts = rim_points(lit, run)
    out, sel = fit_points(pts, h, w, rounds=rounds, min_points=min_points, tol16=tol16)
    rim = np.zeros((len(pts), 3), np.int32)
    if len(pts):
        rim[:, :2] = np.asarray(pts, np.int32)
        rim[:, 2] = sel
    return out, rim
