"""A seeded scene defined on the sphere, rendered into 180-degree equidistant fisheye eyes in NumPy: the input of the rotation-recovery
tests of the feature matcher.  The texture is an equirectangular image of a few thousand axis-aligned rectangles of random grey levels,
0.5 - 4 degrees in size, over low-contrast noise: corners everywhere, no repeating structure (unlike synth.pattern's rings and spokes).
An eye of size n samples the texture bilinearly at each pixel's direction with 2 x 2 supersampling; the right eye of a pair samples at
R d, so a world direction w appears at w in the left eye and at R^T w in the right one."""
from __future__ import annotations

import numpy as np

TEX_DEG_PER_PX = 0.0625
TEX_H, TEX_W = int(180 / TEX_DEG_PER_PX), int(360 / TEX_DEG_PER_PX)
_texture = None


def texture() -> np.ndarray:
    global _texture
    if _texture is None:
        rng = np.random.default_rng(20261016)
        t = (110 + rng.integers(-6, 7, (TEX_H, TEX_W))).astype(np.uint8)
        for _ in range(4000):
            hh, ww = (rng.uniform(0.5, 4.0, 2) / TEX_DEG_PER_PX).astype(int)
            y0, x0 = rng.integers(0, TEX_H - hh), rng.integers(0, TEX_W - ww)
            t[y0:y0 + hh, x0:x0 + ww] = rng.integers(0, 256)
        _texture = t
    return _texture


def rotation(axis, deg: float) -> np.ndarray:
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    th = np.radians(deg)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * k @ k


def _sample(tex: np.ndarray, d: np.ndarray) -> np.ndarray:
    lon = np.arctan2(d[0], d[2])
    lat = np.arcsin(np.clip(d[1], -1, 1))
    tx = (lon + np.pi) / (2 * np.pi) * TEX_W - 0.5
    ty = (lat + np.pi / 2) / np.pi * TEX_H - 0.5
    x0, y0 = np.floor(tx).astype(np.int64), np.floor(ty).astype(np.int64)
    fx, fy = (tx - x0).astype(np.float32), (ty - y0).astype(np.float32)
    xa, xb = x0 % TEX_W, (x0 + 1) % TEX_W
    ya, yb = np.clip(y0, 0, TEX_H - 1), np.clip(y0 + 1, 0, TEX_H - 1)
    t = tex
    top = t[ya, xa] * (1 - fx) + t[ya, xb] * fx
    bot = t[yb, xa] * (1 - fx) + t[yb, xb] * fx
    return top * (1 - fy) + bot * fy


def render(n: int, rot: np.ndarray | None = None) -> np.ndarray:
    """(n, n, 3) BGR uint8 eye, image circle of radius n / 2 about (n // 2, n // 2), black outside"""
    tex = texture().astype(np.float32)
    c, r = n // 2, n / 2
    vv, uu = np.mgrid[:n, :n].astype(np.float32)
    acc = np.zeros((n, n), np.float32)
    inside = np.zeros((n, n), bool)
    for du in (-0.25, 0.25):
        for dv in (-0.25, 0.25):
            x, y = (uu + du - c) / r, (vv + dv - c) / r
            rho = np.hypot(x, y)
            th = rho * (np.pi / 2)
            s = np.where(rho > 0, np.sin(th) / np.maximum(rho, 1e-12), np.pi / 2)
            d = np.stack([s * x, s * y, np.cos(th)])
            if rot is not None:
                d = np.einsum("ij,jhw->ihw", rot.astype(np.float32), d)
            acc += _sample(tex, d)
            inside |= rho <= 1
    img = np.where(inside, np.clip(np.rint(acc / 4), 0, 255), 0).astype(np.uint8)
    return np.repeat(img[..., None], 3, axis=2)


def project(n: int, d: np.ndarray) -> np.ndarray:
    """pixel positions (k, 2) of unit directions (k, 3) in an eye of size n (the inverse of render's mapping)"""
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    th = np.arccos(np.clip(d[:, 2], -1, 1))
    rho = th / (np.pi / 2)
    h = np.maximum(np.hypot(d[:, 0], d[:, 1]), 1e-12)
    return np.stack([n // 2 + n / 2 * rho * d[:, 0] / h, n // 2 + n / 2 * rho * d[:, 1] / h], axis=1)


def directions(k: int, max_deg: float, seed: int = 1) -> np.ndarray:
    """k random unit directions within max_deg of the optical axis"""
    rng = np.random.default_rng(seed)
    th = np.radians(max_deg) * np.sqrt(rng.uniform(0, 1, k))
    ph = rng.uniform(0, 2 * np.pi, k)
    return np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1)
