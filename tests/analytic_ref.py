"""Float64 interpolation from the textbook definitions: what a remap sampler has to compute, stated without OpenCV's tables.

Not a test module: tests/test_analytic_remap.py holds the two restatements of cv2.remap (oracle.remap, wide_ref.remap) to it on the CPU,
tests/test_gpu_analytic.py the HIP samplers.  Nothing here imports the oracle, wide_ref.py or the product: the weights are the hat
function, the Keys cubic convolution kernel (a = -0.75) and sinc(t) sinc(t / 4) on eight taps, the footprint is anchored at
floor(x) - (K / 2 - 1), borders are numpy.pad's, and every sum runs in float64.  What cv2.remap adds to that -- coordinates rounded to
1 / 32 pixel, int16 or float32 weight tables, a rounded and saturated result -- is either applied to the inputs (``quantise``) or
covered by a tolerance derived below (``tolerance``), so a sampler with another kernel shape, anchor, axis order, normalisation or
rounding falls outside it.
"""
from __future__ import annotations

from typing import Any

import numpy as np

INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_LANCZOS4 = 0, 1, 2, 4
BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101 = range(5)
TAPS = {INTER_LINEAR: 2, INTER_CUBIC: 4, INTER_LANCZOS4: 8}
PAD_MODE = {BORDER_REPLICATE: "edge", BORDER_REFLECT: "symmetric", BORDER_WRAP: "wrap", BORDER_REFLECT_101: "reflect"}
COMB_PITCH = 11  # > 8: a footprint meets at most one impulse per axis


# ----------------------------------------------------------------------------------------------------------------------- weights
def hat(f: np.ndarray) -> np.ndarray:
    """(..., 2): max(0, 1 - |t|) at the taps 0, 1 of a sample at fraction f."""
    f = np.asarray(f, np.float64)
    return np.stack([1.0 - f, f], -1)


def keys(t: np.ndarray, a: float = -0.75) -> np.ndarray:
    """Keys' cubic convolution kernel (IEEE Trans. ASSP 29, 1981), free parameter a."""
    t = np.abs(np.asarray(t, np.float64))
    near = ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    far = ((a * t - 5.0 * a) * t + 8.0 * a) * t - 4.0 * a
    return np.where(t <= 1.0, near, np.where(t < 2.0, far, 0.0))


def cubic(f: np.ndarray, a: float = -0.75) -> np.ndarray:
    """(..., 4): the taps -1 .. 2."""
    f = np.asarray(f, np.float64)
    return np.stack([keys(f - k, a) for k in range(-1, 3)], -1)


def lanczos(f: np.ndarray, a: int = 4) -> np.ndarray:
    """(..., 8): sinc(t) sinc(t / a) for |t| < a at the taps -3 .. 4, normalised to sum 1."""
    f = np.asarray(f, np.float64)
    t = np.stack([f - k for k in range(-3, 5)], -1)
    w = np.where(np.abs(t) < a, np.sinc(t) * np.sinc(t / a), 0.0)
    w = np.where((t != 0) & (t == np.rint(t)), 0.0, w)  # sinc's zeros, which sin(pi t) misses by 1e-17
    return w / w.sum(-1, keepdims=True)


def weights(interp: int, f: np.ndarray, mutation: str | None = None) -> np.ndarray:
    if interp == INTER_LINEAR:
        return hat(f)
    if interp == INTER_CUBIC:
        return cubic(f, -0.5 if mutation == "a=-0.5" else -0.75)
    if interp == INTER_LANCZOS4:
        return lanczos(f, 3 if mutation == "lanczos3" else 4)
    raise ValueError(f"no weights for interpolation {interp}")


# ----------------------------------------------------------------------------------------------------------------------- borders
def border_colour(border_value: Any, cn: int) -> np.ndarray:
    """cv2's Scalar: a bare number sets component 0 only, missing components are 0.  The colour is taken as the image stores it: callers
    pass values inside the pixel type's range."""
    vals = [border_value] if np.isscalar(border_value) else list(border_value)
    out = np.zeros(4, np.float64)
    out[: len(vals[:4])] = vals[:4]
    return out[:cn]


def extend(src: np.ndarray, pad: int, border: int, border_value: Any = 0) -> np.ndarray:
    """(H + 2 pad, W + 2 pad, C) float64: the source continued by the border mode (numpy.pad folds as often as it takes)."""
    s = src.astype(np.float64)
    if border == BORDER_CONSTANT:
        out = np.empty((s.shape[0] + 2 * pad, s.shape[1] + 2 * pad, s.shape[2]), np.float64)
        out[...] = border_colour(border_value, s.shape[2])
        out[pad:pad + s.shape[0], pad:pad + s.shape[1]] = s
        return out
    return np.pad(s, ((pad, pad), (pad, pad), (0, 0)), mode=PAD_MODE[border])


def _pad_for(ix: np.ndarray, iy: np.ndarray, h: int, w: int) -> int:
    """the largest excursion of the coordinates from the source, plus 8 (a Lanczos footprint and a moved anchor fit)"""
    if ix.size == 0:
        return 8
    ex = max(0, -int(ix.min()), int(ix.max()) - (w - 1), -int(iy.min()), int(iy.max()) - (h - 1))
    return ex + 8


# ----------------------------------------------------------------------------------------------------------------------- samplers
def sample(src: np.ndarray, x: np.ndarray, y: np.ndarray, interp: int, border: int = BORDER_CONSTANT, border_value: Any = 0, *,
           with_abs: bool = False, mutation: str | None = None):
    """sum over K x K taps of w_y[i] w_x[j] src[floor(y) - (K/2 - 1) + i, floor(x) - (K/2 - 1) + j] in float64, per channel: no rounding,
    no clamping.  ``x``, ``y``: finite float64 arrays of one shape (an image of coordinates or a list of pixels); the result has that
    shape plus the channel axis (none for a 2-D source).  ``with_abs``: also sum |w_i| (same shape as x), sum |w_i p_i| and the largest
    |p_i| of the footprint.
    ``mutation`` makes the reference wrong on purpose, for the tests that show the assertions have teeth: 'a=-0.5', 'lanczos3', 'swap'
    (the weights of fx applied along y and of fy along x), 'anchor' (footprint one tap further left and up)."""
    s = src[..., None] if src.ndim == 2 else src
    h, w, cn = s.shape
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    assert x.shape == y.shape and np.isfinite(x).all() and np.isfinite(y).all()
    ix, iy = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    k = TAPS[interp]
    wx, wy = weights(interp, x - ix, mutation), weights(interp, y - iy, mutation)
    if mutation == "swap":
        wx, wy = wy, wx
    pad = _pad_for(ix, iy, h, w)
    ext = extend(s, pad, border, border_value)
    off = k // 2 - 1 + (1 if mutation == "anchor" else 0)
    x0, y0 = ix - off + pad, iy - off + pad
    acc = np.zeros(x.shape + (cn,), np.float64)
    aw = np.zeros(x.shape, np.float64)
    awp = np.zeros(x.shape + (cn,), np.float64)
    pmax = np.zeros(x.shape + (cn,), np.float64)
    for i in range(k):
        for j in range(k):
            wij = wy[..., i] * wx[..., j]
            p = ext[y0 + i, x0 + j]
            acc += wij[..., None] * p
            if with_abs:
                aw += np.abs(wij)
                awp += np.abs(wij[..., None] * p)
                np.maximum(pmax, np.abs(p), out=pmax)
    if src.ndim == 2:
        acc, awp, pmax = acc[..., 0], awp[..., 0], pmax[..., 0]
    return (acc, aw, awp, pmax) if with_abs else acc


def sum_abs_weights(x: np.ndarray, y: np.ndarray, interp: int) -> np.ndarray:
    """sum |w_i| over the footprint = (sum |w_y|) (sum |w_x|): what ``sample(with_abs=True)`` returns second, without the taps"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return np.abs(weights(interp, y - np.floor(y))).sum(-1) * np.abs(weights(interp, x - np.floor(x))).sum(-1)


def nearest(src: np.ndarray, x: np.ndarray, y: np.ndarray, border: int = BORDER_CONSTANT, border_value: Any = 0) -> np.ndarray:
    """src[rint(y), rint(x)] under the border mode, float64.  For coordinates that are no ties (k + 0.5): the tie rule is cvRound's."""
    s = src[..., None] if src.ndim == 2 else src
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ix, iy = np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)
    pad = _pad_for(ix, iy, s.shape[0], s.shape[1])
    out = extend(s, pad, border, border_value)[iy + pad, ix + pad]
    return out[..., 0] if src.ndim == 2 else out


# ----------------------------------------------------------------------------------------------------------------------- coordinates
def quantise(xm: np.ndarray, ym: np.ndarray):
    """The sampler's one coordinate step, cvRound(map * 32) in float32: (x, y, skip) with x, y = rint(float32(32) * float32 map) / 32 as
    float64 and ``skip`` the pixels to leave out of a comparison -- NaN / infinite entries (the border-value rule for them has its own
    tests) and coordinates beyond +-2^20, where the int16 pixel index of cv2.remap saturates.  Skipped pixels get the coordinate 0."""
    xm, ym = np.asarray(xm, np.float32), np.asarray(ym, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        sx, sy = xm * np.float32(32), ym * np.float32(32)
        skip = ~(np.isfinite(sx) & np.isfinite(sy) & (np.abs(sx) < 2.0 ** 20) & (np.abs(sy) < 2.0 ** 20))
    sx, sy = np.where(skip, 0, sx).astype(np.float64), np.where(skip, 0, sy).astype(np.float64)
    return np.rint(sx) / 32.0, np.rint(sy) / 32.0, skip


def grid_coords(h: int, w: int, ho: int, wo: int, seed: int, margin: int = 5, nearest_safe: bool = False):
    """(x, y) float32 maps of ho x wo random multiples of 1 / 32 from ``margin`` pixels outside the h x w source to its far edge plus
    ``margin``; the first rows and columns walk along every edge from margin outside to margin inside, so that footprints straddle and
    leave the source on all four sides.  ``nearest_safe``: shifted by 1 / 64, so that no coordinate is a rounding tie."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-margin * 32, (w - 1 + margin) * 32 + 1, (ho, wo)).astype(np.float64) / 32
    y = rng.integers(-margin * 32, (h - 1 + margin) * 32 + 1, (ho, wo)).astype(np.float64) / 32
    n = min(wo, 2 * margin * 32 + 1)
    walk = (np.arange(n) - margin * 32) / 32.0
    if ho >= 4:
        x[0, :n], x[1, :n] = walk, (w - 1) - walk  # across the left and the right edge
        y[2, :n], y[3, :n] = walk, (h - 1) - walk  # across the top and the bottom edge
    if nearest_safe:
        x, y = x + 1 / 64, y + 1 / 64
    return x.astype(np.float32), y.astype(np.float32)


def sweep_coords(offsets=range(-4, 5)):
    """All 1024 fraction pairs per integer offset: a (32 n, 32 n) map whose block (a, b) is base + offset[b] + fx / 32 in x and
    base + offset[a] + fy / 32 in y, base = 2 * COMB_PITCH (a lattice point of the comb).  With offsets -4 .. 4 the impulse at the base
    (or a neighbour, 11 pixels on) passes through every tap position of an 8-tap footprint at every fraction pair, fx != fy included."""
    offs = np.asarray(list(offsets), np.float64)
    f = np.arange(32) / 32.0
    line = (2 * COMB_PITCH + offs[:, None] + f[None, :]).reshape(-1)
    x = np.broadcast_to(line[None, :], (line.size, line.size))
    y = np.broadcast_to(line[:, None], (line.size, line.size))
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)


# ----------------------------------------------------------------------------------------------------------------------- sources
def noise(dtype, h: int, w: int, cn: int, seed: int) -> np.ndarray:
    """Seeded noise over the whole range of uint8 / uint16, float32 in [-1, 1]."""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.float32:
        return rng.uniform(-1.0, 1.0, (h, w, cn)).astype(np.float32)
    return rng.integers(0, int(np.iinfo(dtype).max) + 1, (h, w, cn)).astype(dtype)


def comb(h: int, w: int, cn: int, inverse: bool = False, dtype=np.uint8, phase: tuple[int, int] = (0, 0)) -> np.ndarray:
    """255 on a lattice of pitch 11 in both axes, on zero: every output pixel of an 8-tap sampler is 255 wx wy of ONE lattice point, so
    kernel shape, anchor and x / y orientation show undiluted.  ``inverse``: 0 on 255, whose overshoot above 255 meets the upper
    saturation as the comb's negative lobes meet the lower one.  The same values in every channel."""
    a = np.zeros((h, w, cn), dtype)
    a[phase[0]::COMB_PITCH, phase[1]::COMB_PITCH] = 255
    return (255 - a).astype(dtype) if inverse else a


# ----------------------------------------------------------------------------------------------------------------------- tolerances
# uint8 (cv2.remap's fixed point): |got - clip(ref, 0, 255)| <= 0.5 + 255 K^2 / 32768.
#   0.5 is the final rounding (sum + 16384) >> 15.  The K^2 int16 weights are the real ones times 32768, each rounded (<= 0.5 off), and
#   the table's sum fix-up moves minus the sum of those roundings onto one tap: sum |e_i| + |sum e_i| <= K^2 units of 1 / 32768 on
#   pixels <= 255.  Saturation is monotone, so it cannot widen the distance to the clipped reference.
#   = 0.531 (bilinear), 0.625 (bicubic), 0.998 (Lanczos4).  Derived, not measured.
# uint16 (float32 weights, float32 sums, cvRound): 0.5 + 65535 (K^2 + 8) 2^-24 sum |w_i|, per pixel.
#   A term w_i p_i enters the float32 sum with at most K^2 + 8 roundings of relative size 2^-24: seven for the weight (two 1-D weights
#   of at most three roundings each, relative to sum |w| of their axis, and their product), one for the product with the pixel, and at
#   most K^2 for the partial sums it passes through; p_i <= 65535.  sum |w_i| is the 2-D sum (sum |w_y|)(sum |w_x|), at most
#   1 for bilinear, 1.375^2 = 1.89 for bicubic and 1.7146^2 = 2.94 for Lanczos4 (both at fraction 1/2 in both axes): the bound reaches
#   0.547, 0.677 and 1.327 LSB -- above one LSB for Lanczos4 where both fractions are near 1/2, 0.98 where one of them is 0 (UINT16_MAX_TOL,
#   checked by tests/test_analytic_remap.py).  A worst case over every rounding; the restatement's measured maximum is 0.523.
# float32: |got - ref| <= min(F32_REL[interp] * sum |w_i p_i|, F32_PEAK[interp] * sum |w_i| * max |p_i|), per pixel and channel.
#   The summation order is the implementation's, so these are measured: the largest |wide_ref.remap - ref| over either scale on the
#   grid-aligned noise cases of tests/test_analytic_remap.py (float32 noise in [-1, 1], 40 x 60 x 3, 200 x 200 maps, seeds 0 .. 7, a
#   border colour without a zero component), on the CPU, times four.  The first scale alone has a heavy tail: where a footprint crosses
#   the edge cv2.remap sums (p_i - colour) w_i around the border colour, so its rounding goes with the largest tap and not with
#   sum |w_i p_i| (the 5.5e-6 below is ONE pixel of value 0.001 next to a border of 0.25); the second scale, the footprint's largest
#   |p_i| (the border colour's taps included), has no such tail and is the sharp one on ordinary pixels.
F32_REL_MEASURED = {INTER_LINEAR: 1.71e-7, INTER_CUBIC: 5.51e-6, INTER_LANCZOS4: 5.51e-6}
F32_PEAK_MEASURED = {INTER_LINEAR: 1.48e-7, INTER_CUBIC: 3.75e-7, INTER_LANCZOS4: 5.70e-7}  # (max |d|: 1.1e-7, 5.1e-7, 8.6e-7)
F32_REL = {k: 4.0 * v for k, v in F32_REL_MEASURED.items()}
F32_PEAK = {k: 4.0 * v for k, v in F32_PEAK_MEASURED.items()}
# Signed bias: |mean(got - clip(ref))| over a noise case of >= 1e5 samples.  A truncating shift or a floor in place of the rounding shows
#   as -0.5, rounding half away as ~ +0.  Measured on the CPU restatements (oracle.remap for uint8, wide_ref.remap for uint16) over the
#   same cases and seeds, the largest magnitude seen per interpolation; five times that is allowed, 0.05 at the most:
BIAS_MEASURED = {
    np.uint8: {INTER_LINEAR: 0.00583, INTER_CUBIC: 0.00092, INTER_LANCZOS4: 0.00198},  # (bilinear: exact ties are common and round up)
    np.uint16: {INTER_LINEAR: 0.00149, INTER_CUBIC: 0.00182, INTER_LANCZOS4: 0.00202},
}
BIAS_MIN_SAMPLES = 100_000
UINT16_MAX_TOL = {INTER_LINEAR: 0.547, INTER_CUBIC: 0.677, INTER_LANCZOS4: 1.327}  # the uint16 bound at its largest sum |w_i|


def bias_limit(dtype, interp: int) -> float:
    return min(0.05, 5.0 * BIAS_MEASURED[np.dtype(dtype).type][interp])


def tolerance(dtype, interp: int, sum_abs_w: np.ndarray | float = 1.0, sum_abs_wp: np.ndarray | float = 0.0,
              peak: np.ndarray | float = 0.0):
    """The largest |got - expected| allowed, per pixel (see the derivations above); expected = ref clipped to the type's range."""
    k = TAPS[interp]
    dt = np.dtype(dtype)
    if dt == np.uint8:
        return 0.5 + 255.0 * k * k / 32768.0
    if dt == np.uint16:
        return 0.5 + 65535.0 * (k * k + 8) * 2.0 ** -24 * np.asarray(sum_abs_w)
    if dt == np.float32:
        aw = np.asarray(sum_abs_w)
        aw = aw[..., None] if np.ndim(peak) > aw.ndim else aw
        return np.minimum(F32_REL[interp] * np.asarray(sum_abs_wp), F32_PEAK[interp] * aw * np.asarray(peak))
    raise TypeError(dt)


def expected(dtype, ref: np.ndarray) -> np.ndarray:
    """the analytic value as the pixel type can hold it, before rounding: clipped for the integer types"""
    dt = np.dtype(dtype)
    return ref if dt == np.float32 else np.clip(ref, 0, float(np.iinfo(dt).max))


def compare(got: np.ndarray, src: np.ndarray, x, y, interp: int, border: int = BORDER_CONSTANT, border_value: Any = 0, *,
            skip: np.ndarray | None = None, mutation: str | None = None, floor: bool = False) -> dict:
    """Hold ``got`` (the sampler's output at the coordinates x, y: same leading shape) to the analytic value.  Returns the figures of the
    case -- 'excess' = max(|got - expected| - tolerance) (<= 0 passes), 'max' = the largest deviation, 'bias' = mean(got - expected),
    'n' = samples compared -- and asserts nothing.  ``floor``: the mutant whose expected value is rounded down, not to nearest."""
    dt = got.dtype
    g = got.astype(np.float64)
    if interp == INTER_NEAREST:
        ref = nearest(src, x, y, border, border_value)
        tol = np.zeros(ref.shape[: np.ndim(x)])
    else:
        if dt == np.float32:
            ref, aw, awp, peak = sample(src, x, y, interp, border, border_value, with_abs=True, mutation=mutation)
        else:  # (the integer types' bounds need sum |w_i| alone: cheaper on the large GPU cases)
            ref, aw, awp, peak = sample(src, x, y, interp, border, border_value, mutation=mutation), sum_abs_weights(x, y, interp), 0.0, 0.0
        tol = tolerance(dt, interp, aw, awp, peak)
        if dt == np.uint8:
            tol = np.full(aw.shape, tol)
    exp = expected(dt, ref)
    if floor:
        exp = exp - 0.5  # a sampler that rounds to nearest sits 0.5 above one that truncates
    if np.ndim(tol) < g.ndim:
        tol = tol[..., None]
    d = g - exp
    keep = np.ones(d.shape, bool) if skip is None else np.broadcast_to(~skip[..., None] if d.ndim > skip.ndim else ~skip, d.shape)
    dk = d[keep]
    ex = (np.abs(d) - tol)[keep]
    return {"excess": float(ex.max()) if ex.size else 0.0, "max": float(np.abs(dk).max()) if dk.size else 0.0,
            "bias": float(dk.mean()) if dk.size else 0.0, "n": int(dk.size), "bad": int((ex > 0).sum())}
