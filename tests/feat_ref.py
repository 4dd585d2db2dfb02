"""NumPy restatement of the feature pipeline's contract (v1c_feat_detect / v1c_feat_match): every stage from
input bytes to match list, written from the specification and not from the kernels, so that tests can demand bit-exact agreement."""
from __future__ import annotations

import math

import numpy as np

BINS, PAIRS, PATCH = 30, 256, 15
BORDER = PATCH + 1
NO_SECOND = 0x7FFF
DEFAULTS = {"fast_threshold": 20, "margin": 19, "cell": 32, "per_cell": 2, "max_keypoints": 8192, "max_distance": 64, "ratio": (3, 4)}
# the Bresenham circle of radius 3 as (dx, dy), clockwise from the top
CIRCLE = [(0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1),
          (-2, -2), (-1, -3)]
PATTERN_SEED = 0x5EEDF3A7
MASK64 = (1 << 64) - 1


def round_away(v: float) -> int:
    a = math.floor(abs(v) + 0.5)
    return int(-a if v < 0 else a)


# ---- stage 1 ------------------------------------------------------------------------------------------------------------------------
def luma(img: np.ndarray) -> np.ndarray:
    a = np.asarray(img).astype(np.int64)
    if a.ndim == 2:
        return a
    if a.shape[2] == 1:
        return a[..., 0]
    return (1868 * a[..., 0] + 9617 * a[..., 1] + 4899 * a[..., 2] + 8192) >> 14


def working_size(h: int, w: int, s: float) -> tuple[int, int]:
    """(W', H'), as cv2.resize is called by the fm glue"""
    return int(w * s), int(h * s)


def bounds(n_work: int, n: int, s: float) -> np.ndarray:
    return np.array([min(n, math.floor(i / s)) for i in range(n_work + 1)], np.int64)


def resample(img: np.ndarray, s: float) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """working luma image, row boundaries, column boundaries"""
    y = luma(img)
    h, w = y.shape
    ww, wh = working_size(h, w, s)
    rb, cb = bounds(wh, h, s), bounds(ww, w, s)
    cs = np.zeros((h + 1, w + 1), np.int64)
    cs[1:, 1:] = y.cumsum(0).cumsum(1)
    tot = cs[rb[1:, None], cb[None, 1:]] - cs[rb[:-1, None], cb[None, 1:]] - cs[rb[1:, None], cb[None, :-1]] + cs[rb[:-1, None], cb[None, :-1]]
    cnt = (rb[1:] - rb[:-1])[:, None] * (cb[1:] - cb[:-1])[None, :]
    return ((2 * tot + cnt) // (2 * cnt)).astype(np.uint8), rb, cb


# ---- stage 2 ------------------------------------------------------------------------------------------------------------------------
def smooth(y: np.ndarray) -> np.ndarray:
    p = np.pad(y.astype(np.int32), 2, mode="edge")
    h = (p[:, :-4] + 4 * p[:, 1:-3] + 6 * p[:, 2:-2] + 4 * p[:, 3:-1] + p[:, 4:] + 8) >> 4
    v = (h[:-4] + 4 * h[1:-3] + 6 * h[2:-2] + 4 * h[3:-1] + h[4:] + 8) >> 4
    return v.astype(np.uint8)


# ---- stage 3 ------------------------------------------------------------------------------------------------------------------------
def fast_scores(y: np.ndarray) -> np.ndarray:
    """FAST-9 score of every pixel at least 3 pixels inside the image (-256 elsewhere)"""
    a = y.astype(np.int32)
    h, w = a.shape
    c = a[3:h - 3, 3:w - 3]
    d = np.stack([a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in CIRCLE])
    best = np.full(c.shape, -256, np.int32)
    for s in range(16):
        arc = d[[(s + k) % 16 for k in range(9)]]
        best = np.maximum(best, arc.min(0))
        best = np.maximum(best, -arc.max(0))
    out = np.full((h, w), -256, np.int32)
    out[3:h - 3, 3:w - 3] = best
    return out


def disc_ranges(h: int, w: int, s: float, radius: float, margin: int) -> np.ndarray:
    """(lo, hi) qualifying columns of every working row (lo > hi: none); rows and columns within BORDER of the image edge never
    qualify, whatever the radius and the margin"""
    ww, wh = working_size(h, w, s)
    cx, cy = (w // 2) * s, (h // 2) * s
    r = radius * s - margin
    out = np.zeros((wh, 2), np.int64)
    out[:, 0] = 1
    for y in range(wh):
        dy = y - cy
        t = r * r - dy * dy
        if BORDER <= y <= wh - 1 - BORDER and r >= 0 and t >= 0:
            half = math.sqrt(t)
            lo, hi = max(math.ceil(cx - half), BORDER), min(math.floor(cx + half), ww - 1 - BORDER)
            if lo <= hi:
                out[y] = lo, hi
    return out


def candidate_map(y: np.ndarray, ranges: np.ndarray, threshold: int) -> np.ndarray:
    sc = fast_scores(y)
    xx = np.arange(y.shape[1])[None, :]
    inside = (xx >= ranges[:, :1]) & (xx <= ranges[:, 1:])
    return np.where(inside & (sc >= threshold), sc, 0).astype(np.uint8)


# ---- stage 4 ------------------------------------------------------------------------------------------------------------------------
def nms(sc: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(ys, xs) of the candidates that beat every candidate neighbour on (score, -y, -x)"""
    s = sc.astype(np.int32)
    ys, xs = np.nonzero(s)
    c = s[ys, xs]
    keep = np.ones(len(ys), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            v = s[ys + dy, xs + dx]
            before = dy < 0 or (dy == 0 and dx < 0)
            keep &= ~((v > c) | ((v == c) & before))
    return ys[keep], xs[keep]


def select(sc: np.ndarray, cell: int, per_cell: int, max_keypoints: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(xs, ys, scores) of the selected keypoints, cell-major"""
    ys, xs = nms(sc)
    c = sc[ys, xs].astype(np.int64)
    ncx = -(-sc.shape[1] // cell)
    cidx = (ys // cell) * ncx + xs // cell
    o = np.lexsort((xs, ys, -c, cidx))
    xs, ys, c, cidx = xs[o], ys[o], c[o], cidx[o]
    first = np.r_[True, cidx[1:] != cidx[:-1]] if len(cidx) else np.zeros(0, bool)
    starts = np.flatnonzero(first)
    rank = np.arange(len(cidx)) - np.repeat(starts, np.diff(np.r_[starts, len(cidx)]))
    m = rank < per_cell
    xs, ys, c, cidx, rank = xs[m], ys[m], c[m], cidx[m], rank[m]
    if len(c) > max_keypoints:
        keep = np.sort(np.lexsort((rank, cidx, -c))[:max_keypoints])
        xs, ys, c = xs[keep], ys[keep], c[keep]
    return xs, ys, c


# ---- stage 5 ------------------------------------------------------------------------------------------------------------------------
def _splitmix64(state: int) -> tuple[int, int]:
    state = (state + 0x9E3779B97F4A7C15) & MASK64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return state, z ^ (z >> 31)


def base_pattern() -> np.ndarray:
    """256 (px, py, qx, qy): Irwin-Hall (12 uniform 16-bit draws) Gaussian coordinates, sigma 6, both points within radius 13, p != q"""
    state, out = PATTERN_SEED, []
    while len(out) < PAIRS:
        c = []
        for _ in range(4):
            v = -393210
            for _ in range(12):
                state, r = _splitmix64(state)
                v += r >> 48
            n = v * 6
            q = (abs(n) + 32768) // 65536
            c.append(q if n >= 0 else -q)
        if c[0] ** 2 + c[1] ** 2 <= 169 and c[2] ** 2 + c[3] ** 2 <= 169 and (c[0], c[1]) != (c[2], c[3]):
            out.append(c)
    return np.array(out, np.int64)


def pattern() -> np.ndarray:
    """(30, 256, 4) int8: the base pattern rotated by (2k + 1) * 6 degrees, rounded half away from zero"""
    base = base_pattern()
    out = np.zeros((BINS, PAIRS, 4), np.int8)
    for k in range(BINS):
        th = (2 * k + 1) * math.pi / 30
        co, si = math.cos(th), math.sin(th)
        for n in range(PAIRS):
            for e in range(2):
                x, y = float(base[n, 2 * e]), float(base[n, 2 * e + 1])
                out[k, n, 2 * e] = round_away(co * x - si * y)
                out[k, n, 2 * e + 1] = round_away(si * x + co * y)
    return out


def bin_vectors() -> np.ndarray:
    return np.array([(round_away(32768.0 * math.cos(k * math.pi / 15)), round_away(32768.0 * math.sin(k * math.pi / 15)))
                     for k in range(BINS)], np.int64)


DISC = [(dx, dy) for dy in range(-PATCH, PATCH + 1) for dx in range(-PATCH, PATCH + 1) if dx * dx + dy * dy <= PATCH * PATCH]


def moments(sm: np.ndarray, xs: np.ndarray, ys: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    dx = np.array([d[0] for d in DISC])
    dy = np.array([d[1] for d in DISC])
    v = sm[ys[:, None] + dy[None], xs[:, None] + dx[None]].astype(np.int64)
    return (v * dx).sum(1), (v * dy).sum(1)


def orient_bins(m10: np.ndarray, m01: np.ndarray) -> np.ndarray:
    bv = bin_vectors()
    cr = bv[None, :, 0] * m01[:, None] - bv[None, :, 1] * m10[:, None]  # cross(b_k, m)
    ok = (cr >= 0) & (np.roll(cr, -1, axis=1) < 0)
    return np.where(ok.any(1), ok.argmax(1), 0)


def descriptors(sm: np.ndarray, xs: np.ndarray, ys: np.ndarray, bins: np.ndarray, pat: np.ndarray | None = None) -> np.ndarray:
    p = (pattern() if pat is None else pat)[bins].astype(np.int64)
    a = sm[ys[:, None] + p[..., 1], xs[:, None] + p[..., 0]]
    b = sm[ys[:, None] + p[..., 3], xs[:, None] + p[..., 2]]
    return np.packbits(a < b, axis=1, bitorder="little")


def detect(img: np.ndarray, *, radius: float, scale: float = 1.0, **overrides) -> tuple[np.ndarray, np.ndarray]:
    """(N, 6) int32 keypoints (x, y, score, bin, src_x2, src_y2) and (N, 32) uint8 descriptors, as v1c_feat_detect"""
    p = {**DEFAULTS, **overrides}
    img = np.asarray(img)
    h, w = img.shape[:2]
    y, rb, cb = resample(img, scale)
    sm = smooth(y)
    sc = candidate_map(y, disc_ranges(h, w, scale, radius, p["margin"]), p["fast_threshold"])
    xs, ys, c = select(sc, p["cell"], p["per_cell"], p["max_keypoints"])
    m10, m01 = moments(sm, xs, ys)
    bins = orient_bins(m10, m01)
    kp = np.stack([xs, ys, c, bins, cb[xs] + cb[xs + 1] - 1, rb[ys] + rb[ys + 1] - 1], axis=1).astype(np.int32).reshape(-1, 6)
    return kp, descriptors(sm, xs, ys, bins).reshape(-1, 32)


# ---- stage 6 ------------------------------------------------------------------------------------------------------------------------
def distances(d1: np.ndarray, d2: np.ndarray) -> np.ndarray:
    a, b = np.ascontiguousarray(d1).view(np.uint64), np.ascontiguousarray(d2).view(np.uint64)
    out = np.zeros((len(a), len(b)), np.int32)
    for k in range(4):
        out += np.bitwise_count(a[:, k, None] ^ b[None, :, k])
    return out


def best(d: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """per row: best distance, its (lowest) index, second-best distance (NO_SECOND with one column)"""
    idx = d.argmin(1)
    d1 = d[np.arange(len(d)), idx]
    d2 = np.partition(d, 1, axis=1)[:, 1] if d.shape[1] > 1 else np.full(len(d), NO_SECOND)
    return d1, idx, d2


def match(desc1: np.ndarray, desc2: np.ndarray, max_distance: int = 64, ratio: tuple[int, int] = (3, 4)):
    """(idx1, idx2, dist) as v1c_feat_match"""
    if len(desc1) == 0 or len(desc2) == 0:
        e = np.zeros(0, np.int64)
        return e, e, e
    d = distances(desc1, desc2)
    d1, i12, d2 = best(d)
    _, i21, _ = best(d.T)
    num, den = ratio
    i = np.arange(len(d))
    keep = (i21[i12] == i) & (d1 <= max_distance) & (den * d1 <= num * d2)
    return i[keep], i12[keep], d1[keep]


# ---- stage 6 for large sets: the same rule, the distances a block of rows at a time --------------------------------------------------
BLOCK_BYTES = 64 << 20  # the int32 distances held at a time (`distances` of 17000 x 9000 descriptors would take ~2 GB with its temporaries)


def _two_smallest(d: np.ndarray, axis: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """along `axis`: smallest value, its lowest index, second-smallest value (NO_SECOND with one entry); `d` comes back unchanged"""
    idx = d.argmin(axis)
    at = (np.arange(d.shape[0]), idx) if axis == 1 else (idx, np.arange(d.shape[1]))
    d1 = d[at]
    if d.shape[axis] == 1:
        return d1, idx, np.full(len(d1), NO_SECOND, np.int64)
    d[at] = NO_SECOND
    d2 = d.min(axis)
    d[at] = d1
    return d1, idx, d2.astype(np.int64)


def best_both(desc1: np.ndarray, desc2: np.ndarray, block_bytes: int = BLOCK_BYTES):
    """((d1, idx, d2) of every row, (d1, idx, d2) of every column) of the distance matrix, which is never held whole: blocks of rows of
    at most `block_bytes`, the rows' results block by block and a running best / lowest index / second best of every column.  Both sets
    non-empty."""
    na, nb = len(desc1), len(desc2)
    step = max(1, block_bytes // (4 * nb))
    rows = [np.zeros(na, np.int64) for _ in range(3)]
    c1, ci, c2 = np.full(nb, NO_SECOND, np.int64), np.full(nb, -1, np.int64), np.full(nb, NO_SECOND, np.int64)
    for r0 in range(0, na, step):
        d = distances(desc1[r0:r0 + step], desc2)
        for out, v in zip(rows, _two_smallest(d, 1)):
            out[r0:r0 + step] = v
        b1, bi, b2 = _two_smallest(d, 0)
        # this block's rows come after every earlier one: only a strictly smaller distance takes the column over
        take = b1 < c1
        c2 = np.where(take, np.minimum(c1, b2), np.minimum(b1, c2))
        ci = np.where(take, bi + r0, ci)
        c1 = np.where(take, b1, c1)
    return tuple(rows), (c1, ci, c2)


def match_from_best(rows, cols, max_distance: int = 64, ratio: tuple[int, int] = (3, 4)):
    """the match rule on `best_both`'s results (swap them for the other argument order)"""
    d1, i12, d2 = rows
    num, den = ratio
    i = np.arange(len(d1))
    keep = (cols[1][i12] == i) & (d1 <= max_distance) & (den * d1 <= num * d2)
    return i[keep], i12[keep], d1[keep]


def match_blocked(desc1: np.ndarray, desc2: np.ndarray, max_distance: int = 64, ratio: tuple[int, int] = (3, 4),
                  block_bytes: int = BLOCK_BYTES):
    """`match`, with at most `block_bytes` of distances in memory"""
    if len(desc1) == 0 or len(desc2) == 0:
        e = np.zeros(0, np.int64)
        return e, e, e
    return match_from_best(*best_both(desc1, desc2, block_bytes), max_distance, ratio)


# ---- what v1c_feat_detect refuses -----------------------------------------------------------------------------------------------------
def refusal(h: int, w: int, scale: float, radius: float, margin: int) -> str | None:
    """why v1c_feat_detect answers V1C_E_INVALID for an (h, w) image with in-range parameters, or None where it runs: a working image
    under 33 x 33, an empty source block, or no qualifying pixel"""
    ww, wh = working_size(h, w, scale)
    if ww < 2 * BORDER + 1 or wh < 2 * BORDER + 1:
        return "working image under 33 x 33"
    if (np.diff(bounds(wh, h, scale)) <= 0).any() or (np.diff(bounds(ww, w, scale)) <= 0).any():
        return "empty source block"
    rg = disc_ranges(h, w, scale, radius, margin)
    if not (rg[:, 0] <= rg[:, 1]).any():
        return "empty circle"
    return None
