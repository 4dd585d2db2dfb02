"""NumPy restatement of the vignetting correction's device rule (``v1c_vignette_apply_async`` /
``v1c_vignette_rings_async``): the exact squared distance, the fixed-point table position, the interpolated Q14 gain, the rounded
product, and the ring statistics.  Integer arithmetic from end to end (uint64 where a product passes 63 bits; it stays below 2^64),
written for reading, not for speed: the device is held to it byte for byte.

The float64 step in front of it (``gain_tables``, ``table_scale``) is the package's own host code and is tested against float64
separately (tests/test_vignette_host.py)."""
import numpy as np

BINS = 1024


def r2_of(h, w, cx, cy):
    """(h, w) int64: (x - cx)^2 + (y - cy)^2, exact (below 2^34 for every frame and centre the entries accept)"""
    dx = np.arange(w, dtype=np.int64) - int(cx)
    dy = np.arange(h, dtype=np.int64) - int(cy)
    return dx[None, :] ** 2 + dy[:, None] ** 2


def position(r2, scale, shift):
    """(idx, f): q = (r2 * scale) >> shift has 8 fraction bits; idx = q >> 8 and f = q & 255, the last interval held beyond the table"""
    assert 0 <= int(r2.min()) and int(r2.max()) < 1 << 34 and 0 < int(scale) < 1 << 30 and 0 <= int(shift) <= 62
    q = (r2.astype(np.uint64) * np.uint64(scale)) >> np.uint64(shift)  # (below 2^64: exact in uint64)
    i = q >> np.uint64(8)
    beyond = i >= BINS
    idx = np.where(beyond, BINS - 1, i).astype(np.int64)
    f = np.where(beyond, 255, q & np.uint64(255)).astype(np.int64)
    return idx, f


def gains_q14(tables, idx, f):
    """(3, h, w) int64: G = (T[idx] (256 - f) + T[idx + 1] f + 128) >> 8"""
    T = np.asarray(tables).astype(np.int64)
    assert T.shape == (3, BINS + 1)
    return (T[:, idx] * (256 - f) + T[:, idx + 1] * f + 128) >> 8


def apply(image, tables, cx, cy, scale, shift):
    """out = min(maxv, (v G + 2^13) >> 14) on the colour channels (BGR tables); a fourth channel is copied, a grey image takes the green
    table"""
    a = image if image.ndim == 3 else image[..., None]
    assert a.dtype in (np.uint8, np.uint16) and a.shape[2] in (1, 3, 4)
    maxv = 255 if a.dtype == np.uint8 else 65535
    h, w, cn = a.shape
    G = gains_q14(tables, *position(r2_of(h, w, cx, cy), scale, shift))
    out = a.copy()
    for c in range(1 if cn == 1 else 3):
        g = G[1] if cn == 1 else G[c]
        out[..., c] = np.minimum(maxv, (a[..., c].astype(np.int64) * g + (1 << 13)) >> 14).astype(a.dtype)
    return out.reshape(image.shape)


def rings(image, cx, cy, R2, nrings, lo, hi):
    """(nrings, 4) int64 (sumB, sumG, sumR, n): over the pixels with r2 < R2 whose colour channels all lie in [lo, hi],
    ring = min(nrings - 1, (r2 * nrings) // R2).  A grey image fills sumG only."""
    a = image if image.ndim == 3 else image[..., None]
    assert a.dtype in (np.uint8, np.uint16) and a.shape[2] in (1, 3, 4)
    h, w, cn = a.shape
    cc = 1 if cn == 1 else 3
    r2 = r2_of(h, w, cx, cy)
    col = a[..., :cc].astype(np.int64)
    m = (r2 < int(R2)) & (col.min(axis=2) >= lo) & (col.max(axis=2) <= hi)
    ring = np.minimum(nrings - 1, (r2[m] * int(nrings)) // int(R2))
    out = np.zeros((nrings, 4), np.int64)
    for c in range(cc):
        np.add.at(out[:, 1 if cn == 1 else c], ring, col[..., c][m])
    np.add.at(out[:, 3], ring, 1)
    return out
