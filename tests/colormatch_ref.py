"""NumPy restatement of the colour match of the two eyes (``v1c_color_match_luts_async`` /
``v1c_apply_luts_async``): the joint mask, the per-channel histograms, the 256-entry tables of both modes, the report record and the
apply step.  Integer arithmetic from end to end (Python ints where a product could pass 64 bits), written for reading, not for speed:
the device is held to it byte for byte."""
import numpy as np

DEFAULTS = dict(mode="histogram", reference="left", lo=10, hi=254, max_shift=64, min_pixels=1024)
MODES = {"histogram": 0, "gain": 1}
REFERENCES = {"left": 0, "right": 1}
G_MIN, G_MAX, G_ONE = 16384, 262144, 65536
REPORT_WORDS = 20  # status, n, then per colour channel: first / last populated bin of the left eye, of the right eye, g; two spare


def _colour(img):
    a = img if img.ndim == 3 else img[..., None]
    assert a.dtype == np.uint8 and a.shape[2] in (1, 3, 4)
    return a, (1 if a.shape[2] == 1 else 3)


def mask(left, right, lo=10, hi=254):
    """positions whose maximum over the colour channels lies in [lo, hi] in BOTH eyes"""
    (a, nc), (b, _) = _colour(left), _colour(right)
    assert a.shape == b.shape
    ma, mb = a[..., :nc].max(axis=2), b[..., :nc].max(axis=2)
    return (ma >= lo) & (ma <= hi) & (mb >= lo) & (mb <= hi)


def histograms(left, right, lo=10, hi=254):
    """h[eye][c][v] (uint32, eye 0 = left; channels a 1-channel image lacks stay zero) and n"""
    (a, nc), (b, _) = _colour(left), _colour(right)
    assert a.shape[0] * a.shape[1] < 2 ** 31
    m = mask(left, right, lo, hi)
    h = np.zeros((2, 3, 256), np.uint32)
    for e, im in enumerate((a, b)):
        for c in range(nc):
            h[e, c] = np.bincount(im[..., c][m], minlength=256)
    return h, int(m.sum())


def histogram_lut(T, R, max_shift=64):
    """the table that maps the distribution T onto R: mid-rank knots at T's populated bins, rounded linear interpolation between them"""
    T, R = [int(v) for v in T], [int(v) for v in R]
    CT, CR = np.cumsum(T).tolist(), np.cumsum(R).tolist()
    knots = []
    for v in range(256):
        if T[v]:
            mid2 = (CT[v - 1] if v else 0) + CT[v]
            knots.append((v, min(u for u in range(256) if 2 * CR[u] >= mid2)))
        elif v in (0, 255):
            knots.append((v, v))
    m = [0] * 256
    for (a, ma), (b, mb) in zip(knots, knots[1:]):
        for v in range(a, b):
            m[v] = ma + ((v - a) * (mb - ma) * 2 + (b - a)) // (2 * (b - a))
    m[255] = knots[-1][1]
    return np.array([min(255, max(0, min(v + max_shift, max(v - max_shift, m[v])))) for v in range(256)], np.uint8)


def gain_of(T, R):
    """g in 1/65536, None where the target's sum is zero"""
    sT, sR = sum(v * int(T[v]) for v in range(256)), sum(v * int(R[v]) for v in range(256))
    if sT == 0:
        return None
    return min(G_MAX, max(G_MIN, (sR * G_ONE + sT // 2) // sT))


def gain_lut(g):
    return np.array([min(255, (v * g + 32768) >> 16) for v in range(256)], np.uint8)


def _ends(hist):
    nz = np.flatnonzero(hist)
    return (int(nz[0]), int(nz[-1])) if len(nz) else (-1, -1)


def luts(left, right, *, mode="histogram", reference="left", lo=10, hi=254, max_shift=64, min_pixels=1024):
    """(luts (3, 256) uint8, report (20,) int32, histograms): the tables that map the eye that is NOT the reference onto the reference"""
    h, n = histograms(left, right, lo, hi)
    nc = _colour(left)[1]
    ref = REFERENCES[reference]
    tgt = 1 - ref
    gains = [gain_of(h[tgt, c], h[ref, c]) if mode == "gain" else None for c in range(nc)]
    status = 1 if n < min_pixels else 2 if mode == "gain" and any(g is None for g in gains) else 0
    out = np.tile(np.arange(256, dtype=np.uint8), (3, 1))
    report = np.zeros(REPORT_WORDS, np.int32)
    report[0], report[1] = status, n
    for c in range(3):
        if c < nc:
            report[2 + 5 * c: 6 + 5 * c] = _ends(h[0, c]) + _ends(h[1, c])
            report[6 + 5 * c] = (gains[c] or 0) if mode == "gain" else 0
            if status == 0:
                out[c] = gain_lut(gains[c]) if mode == "gain" else histogram_lut(h[tgt, c], h[ref, c], max_shift)
        else:
            report[2 + 5 * c: 6 + 5 * c] = -1
    return out, report, h


def apply_luts(image, luts):
    """out[c] = LUT[c][image[c]] on the colour channels; a fourth channel is copied"""
    a, nc = _colour(image)
    out = a.copy()
    for c in range(nc):
        out[..., c] = luts[c][a[..., c]]
    return out.reshape(image.shape)


def match_eyes(left, right, **kw):
    """(the rewritten target eye, luts, report); the reference eye is untouched"""
    p = dict(DEFAULTS, **kw)
    t, report, _ = luts(left, right, **p)
    return apply_luts(right if p["reference"] == "left" else left, t), t, report
