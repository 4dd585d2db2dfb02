"""Independent NumPy restatement of cv2.remap for CV_16U and CV_32F images ("16-bit and float32 images").

Not a test module: tests/test_wide_host.py and tests/test_gpu_wide.py compare the product against it.  Nothing here calls the product:
the float weight table is computed from the 1-D formulas of OpenCV's interpolation tables, the samplers follow the contract operation by
operation (float32 throughout, no fused multiply-add, left-to-right sums) and work on whole maps at once.
"""
from __future__ import annotations

import math
from typing import Any

import numpy as np

INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA, INTER_LANCZOS4 = 0, 1, 2, 3, 4
BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101, BORDER_TRANSPARENT = range(6)
INT_MIN = -(2 ** 31)
F = np.float32


def taps_per_axis(interp: int) -> int:
    return {INTER_LINEAR: 2, INTER_CUBIC: 4, INTER_LANCZOS4: 8}[interp]


def t1d(interp: int) -> np.ndarray:
    """(32, K) float32: the 1-D weights of the fractions 0/32 .. 31/32."""
    K = taps_per_axis(interp)
    out = np.zeros((32, K), F)
    for i in range(32):
        x = F(i) * F(1.0 / 32)
        if interp == INTER_LINEAR:
            out[i] = [F(1) - x, x]
        elif interp == INTER_CUBIC:
            A = F(-0.75)
            x1, one = x + F(1), F(1)
            c0 = ((A * x1 - F(5) * A) * x1 + F(8) * A) * x1 - F(4) * A
            c1 = ((A + F(2)) * x - (A + F(3))) * x * x + one
            c2 = ((A + F(2)) * (one - x) - (A + F(3))) * (one - x) * (one - x) + one
            c3 = one - c0 - c1 - c2
            out[i] = [c0, c1, c2, c3]
        else:
            if x < F(1.1920928955078125e-07):
                out[i] = [0, 0, 0, 1, 0, 0, 0, 0]
                continue
            s45 = 0.70710678118654752440084436210485
            cs = [(1, 0), (-s45, -s45), (0, 1), (s45, -s45), (-1, 0), (s45, s45), (0, -1), (-s45, s45)]
            y0 = -float(x + F(3)) * math.pi * 0.25
            s0, co0 = math.sin(y0), math.cos(y0)
            c = []
            total = F(0)
            for k in range(8):
                y = -float(x + F(3) - F(k)) * math.pi * 0.25
                c.append(F((cs[k][0] * s0 + cs[k][1] * co0) / (y * y)))
                total = F(total + c[-1])
            inv = F(F(1) / total)
            out[i] = [F(v * inv) for v in c]
    return out


def ftab(interp: int) -> np.ndarray:
    """(1024, K, K) float32: wf[fy * 32 + fx][k1][k2] = t1d[fy][k1] * t1d[fx][k2], no sum fix-up."""
    t = t1d(interp)
    K = t.shape[1]
    w = (t[:, None, :, None] * t[None, :, None, :]).astype(F)  # [fy, fx, k1, k2]
    return w.reshape(1024, K, K)


def border_cval(value: Any, dtype) -> np.ndarray:
    """cv2 Scalar -> float32[4] of the saturated border colour of a `dtype` image (a bare number sets component 0 only)."""
    vals = [value] if np.isscalar(value) else list(value)
    out = np.zeros(4, F)
    for i, v in enumerate(vals[:4]):
        v = float(v)
        if np.dtype(dtype) == np.uint16:
            r = INT_MIN if not (abs(v) < 2.0 ** 31) else int(np.rint(v))  # cvRound(double): half to even
            out[i] = min(65535, max(0, r))
        else:
            out[i] = F(v)
    return out


def _cv_round(v: np.ndarray) -> np.ndarray:
    v = v.astype(F)
    with np.errstate(invalid="ignore"):
        ok = np.abs(v) < F(2.0 ** 31)
    return np.where(ok, np.rint(np.where(ok, v, 0)), INT_MIN).astype(np.int64)


def border_index(p: np.ndarray, n: int, border: int) -> np.ndarray:
    """cv::borderInterpolate, -1 for BORDER_CONSTANT / TRANSPARENT outside the image."""
    inside = (p >= 0) & (p < n)
    if border == BORDER_REPLICATE:
        q = np.clip(p, 0, n - 1)
    elif border == BORDER_REFLECT_101:
        if n == 1:
            q = np.zeros_like(p)
        else:
            per = 2 * (n - 1)
            q = np.abs(p) % per
            q = np.where(q >= n, per - q, q)
    elif border == BORDER_REFLECT:
        per = 2 * n
        q = p % per
        q = np.where(q >= n, per - 1 - q, q)
    elif border == BORDER_WRAP:
        q = p % n
    else:
        q = np.full_like(p, -1)
    return np.where(inside, p, q)


def _cast(v: np.ndarray, dtype) -> np.ndarray:
    if np.dtype(dtype) == np.uint16:
        return np.clip(_cv_round(v), 0, 65535).astype(np.uint16)
    return v.astype(F)


def remap(src: np.ndarray, xmap: np.ndarray, ymap: np.ndarray, interp: int, border: int, border_value: Any = 0,
          dst: np.ndarray | None = None) -> np.ndarray:
    """cv2.remap(src, xmap, ymap, interp, borderMode=border, borderValue=border_value) of a uint16 / float32 (H, W[, C]) image;
    pixels that BORDER_TRANSPARENT skips keep `dst`'s value (zeros when None)."""
    with np.errstate(invalid="ignore", over="ignore"):  # (Inf - Inf, Inf * 0: NaN, as in the float32 arithmetic restated)
        return _remap(src, xmap, ymap, interp, border, border_value, dst)


def _remap(src, xmap, ymap, interp, border, border_value, dst):
    dtype = src.dtype
    assert dtype in (np.uint16, np.float32)
    s = src if src.ndim == 3 else src[..., None]
    H, W, cn = s.shape
    xmap, ymap = np.asarray(xmap, F), np.asarray(ymap, F)
    Hd, Wd = xmap.shape
    out = np.zeros((Hd, Wd, cn), dtype) if dst is None else (dst if dst.ndim == 3 else dst[..., None]).copy()
    cv = border_cval(border_value, dtype)[:cn]
    p = s.astype(F)
    if interp == INTER_AREA:
        interp = INTER_LINEAR
    keep = np.zeros((Hd, Wd), bool)  # TRANSPARENT: leave untouched

    def gather(yi, xi):  # (..) index arrays -> (.., cn) float32, indices < 0 -> cval
        ok = (yi >= 0) & (xi >= 0)
        v = p[np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)]
        return np.where(ok[..., None], v, cv)

    if interp == INTER_NEAREST:
        ix = np.clip(_cv_round(xmap), -32768, 32767)
        iy = np.clip(_cv_round(ymap), -32768, 32767)
        inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        if border == BORDER_TRANSPARENT:
            keep = ~inside
        v = gather(border_index(iy, H, border), border_index(ix, W, border))
        res = _cast(v, dtype)
    else:
        sx = _cv_round(xmap * F(32))
        sy = _cv_round(ymap * F(32))
        ix, iy = np.clip(sx >> 5, -32768, 32767), np.clip(sy >> 5, -32768, 32767)
        fx, fy = sx & 31, sy & 31
        if interp == INTER_LINEAR:
            tx1 = fx.astype(F) * F(1.0 / 32)
            ty1 = fy.astype(F) * F(1.0 / 32)
            tx0, ty0 = F(1) - tx1, F(1) - ty1
            w = [(ty0 * tx0)[..., None], (ty0 * tx1)[..., None], (ty1 * tx0)[..., None], (ty1 * tx1)[..., None]]
            inl = (ix >= 0) & (ix < W - 1) & (iy >= 0) & (iy < H - 1)
            x0, x1 = border_index(ix, W, border), border_index(ix + 1, W, border)
            y0, y1 = border_index(iy, H, border), border_index(iy + 1, H, border)
            v = ((gather(y0, x0) * w[0] + gather(y0, x1) * w[1]) + gather(y1, x0) * w[2]) + gather(y1, x1) * w[3]
            res = _cast(v, dtype)
            if border == BORDER_CONSTANT:
                far = (ix >= W) | (ix + 1 < 0) | (iy >= H) | (iy + 1 < 0)
                res = np.where((far & ~inl)[..., None], _cast(np.broadcast_to(cv, v.shape), dtype), res)
            if border == BORDER_TRANSPARENT:
                keep = ~inl
        else:
            K = taps_per_axis(interp)
            wt = ftab(interp)[fy * 32 + fx]  # (Hd, Wd, K, K)
            off = K // 2 - 1
            ox, oy = ix - off, iy - off
            inl = (ox >= 0) & (ox < max(W - (K - 1), 0)) & (oy >= 0) & (oy < max(H - (K - 1), 0))
            eff = border
            if border == BORDER_TRANSPARENT:
                keep = ~inl & ((ix < 0) | (ix >= W) | (iy < 0) | (iy >= H))
                eff = BORDER_REFLECT_101
            # inlier footprint: each row one left-to-right sum, rows added (cubic from R0, Lanczos4 from 0)
            xs_in = [np.clip(ox + j, 0, W - 1) for j in range(K)]
            total = None
            for i in range(K):
                yi = np.clip(oy + i, 0, H - 1)
                r = None
                for j in range(K):
                    t = p[yi, xs_in[j]] * wt[..., i, j][..., None]
                    r = t if r is None else r + t
                if total is None:
                    total = r if K == 4 else F(0) + r
                else:
                    total = total + r
            # other pixels: cv + sum over the valid taps of (p - cv) * w, row-major
            xs = [border_index(ox + j, W, eff) for j in range(K)]
            acc = np.broadcast_to(cv, (Hd, Wd, cn)).astype(F)
            for i in range(K):
                yi = border_index(oy + i, H, eff)
                for j in range(K):
                    ok = ((yi >= 0) & (xs[j] >= 0))[..., None]
                    t = p[np.clip(yi, 0, H - 1), np.clip(xs[j], 0, W - 1)]
                    acc = np.where(ok, acc + (t - cv) * wt[..., i, j][..., None], acc)
            v = np.where(inl[..., None], total, acc)
            res = _cast(v, dtype)
            if eff == BORDER_CONSTANT:
                far = (ox >= W) | (ox + K <= 0) | (oy >= H) | (oy + K <= 0)
                res = np.where((far & ~inl)[..., None], _cast(np.broadcast_to(cv, v.shape), dtype), res)
    out = np.where(keep[..., None], out, res)
    return out if src.ndim == 3 else out[..., 0]
