"""The boundary images of the device JPEG encoder, shared by the host half (tests/test_jpeg_device_host.py: the product's arithmetic on
the CPU against the restatement, and the proof that the list holds what it is for) and the GPU half (tests/test_gpu_jpeg_edges.py: the
kernels against the same bytes).  Every case is a fraction of a second; the restatement of each is computed once and shared."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import jpg_ref as R


class Case(NamedTuple):
    base: np.ndarray       # the 1-D uint8 buffer the image lies in
    offset: int            # byte of the image's first pixel
    h: int
    w: int
    cn: int
    pitch: int             # bytes from one row to the next
    quality: int
    subsampling: str
    restart: int

    def image(self) -> np.ndarray:
        """the (h, w, cn) view of the buffer: pitched rows, dense pixels"""
        return np.lib.stride_tricks.as_strided(self.base[self.offset:], (self.h, self.w, self.cn), (self.pitch, self.cn, 1), writeable=False)


def dense(img, quality=95, subsampling="420", restart=None) -> Case:
    a = np.ascontiguousarray(img if img.ndim == 3 else img[..., None])
    h, w, cn = a.shape
    restart = R.default_restart_mcus(h, w, cn, subsampling) if restart is None else restart
    return Case(a.reshape(-1), 0, h, w, cn, w * cn, quality, subsampling, restart)


def window(whole, x0, w, lead=0, **kw) -> Case:
    """columns [x0, x0 + w) of a wider image, the buffer shifted by ``lead`` bytes (an odd lead: a misaligned pointer)"""
    c = dense(whole, **kw)
    base = np.concatenate([np.full(lead, 0xA5, np.uint8), c.base])
    restart = kw.get("restart") or R.default_restart_mcus(c.h, w, c.cn, c.subsampling)
    return c._replace(base=base, offset=lead + x0 * c.cn, w=w, restart=restart)


def smooth(h, w, cn, seed):
    """a natural-looking image: low-frequency waves and a little noise"""
    rng = R._rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for _ in range(cn):
        fx, fy, ph = rng.uniform(0.02, 0.4, 2).tolist() + [rng.uniform(0, 6)]
        out.append(128 + 90 * np.sin(fx * x + fy * y + ph) + rng.normal(0, 6, (h, w)))
    return np.clip(np.stack(out, axis=-1), 0, 255).astype(np.uint8)


def noise(h, w, cn, seed):
    return R._rng(seed).integers(0, 256, (h, w, cn), dtype=np.uint8)


def _basis():
    k = np.arange(8)
    c = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k[:, None] == 0, np.sqrt(0.5), 1.0) / 2
    return c  # c[u, x]


def from_coefficients(blocks, quality):
    """a grey image of 8 x 8 blocks side by side whose quantised coefficients are ``blocks`` (each {zigzag position: value}): the inverse
    DCT of the dequantised values, rounded.  Meant for coarse tables, where the rounding of the pixels stays far below a step."""
    q = R.quant_table(R.Q_LUMA, quality)
    c = _basis()
    out = []
    for blk in blocks:
        f = np.zeros(64)
        for k, v in blk.items():
            f[R.ZIGZAG[k]] = v * q[R.ZIGZAG[k]]
        px = c.T @ f.reshape(8, 8) @ c + 128
        assert px.min() >= 0 and px.max() <= 255
        out.append(np.rint(px).astype(np.uint8))
    return np.concatenate(out, axis=1)


def swing():
    """full swing at quality 100: a white block beside a black one (a DC difference of category 11) and blocks cut by an edge (AC
    coefficients of category 10)"""
    a = np.zeros((16, 32), np.uint8)
    a[0:8, 0:8] = 255
    a[0:8, 20:24] = 255
    a[12:16, 0:8] = 255
    a[8:16, 16:32] = (np.indices((8, 16)).sum(0) % 2) * 255
    a[0:8, 24:32] = 255
    return a


SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 17), (15, 33), (31, 16)]
PAD_SEED = 3  # noise whose 64 one-block intervals include some of a multiple of 8 bits and some whose padded last byte is 0xFF


@functools.lru_cache(maxsize=None)
def shared_cases() -> dict:
    c = {}
    for i, (h, w) in enumerate(SIZES):
        for sub in ("420", "444"):
            c[f"size_{h}x{w}_{sub}"] = dense(smooth(h, w, 3, 10 + i), 95, sub)
        c[f"size_{h}x{w}_gray"] = dense(smooth(h, w, 1, 30 + i), 95)
    # 5 x 3 MCUs of 16: three MCUs per interval end mid-row; 9 x 5 MCUs of 8 with one or two per interval: RSTm wraps
    c["midrow_420_r3"] = dense(smooth(40, 72, 3, 50), 95, "420", 3)
    c["midrow_444_r7"] = dense(smooth(40, 72, 3, 51), 95, "444", 7)
    c["restart1_444"] = dense(smooth(40, 72, 3, 52), 95, "444", 1)
    c["restart2_420"] = dense(smooth(96, 112, 3, 53), 95, "420", 2)
    c["restart_exact"] = dense(smooth(40, 72, 3, 54), 95, "420", 15)
    c["restart_more"] = dense(smooth(40, 72, 3, 55), 95, "420", 16)
    c["restart_max"] = dense(smooth(24, 24, 1, 56), 95, "420", 65535)
    c["flat"] = dense(np.full((24, 40, 3), 128, np.uint8), 95, "420", 2)
    c["flat_gray_200"] = dense(np.full((9, 17), 200, np.uint8), 50)
    c["only_63"] = dense(from_coefficients([{63: 2}, {63: -1}, {0: 3, 63: 1}], 50), 50, restart=1)
    c["zero_runs"] = dense(from_coefficients([{16: 1, 33: -1, 51: 1}, {34: 1}, {17: -1, 35: 1}, {0: -2, 1: 1, 63: 1}], 50), 50, restart=4)
    c["swing_q100"] = dense(swing(), 100)
    c["noise_q100_444"] = dense(noise(32, 48, 3, 60), 100, "444", 2)
    c["noise_q100_420"] = dense(noise(33, 47, 3, 61), 100, "420", 1)
    c["noise_gray_q100_r1"] = dense(noise(64, 64, 1, PAD_SEED), 100, restart=1)
    for q in (1, 49, 50, 95, 100):
        c[f"quality_{q}"] = dense(smooth(33, 47, 3, 70 + q), q, "420", 2)
    c["bgra"] = dense(noise(20, 36, 4, 80) // 2 + smooth(20, 36, 4, 81) // 2, 95, "420", 2)
    c["bgra_444"] = dense(smooth(20, 36, 4, 82), 90, "444", 3)
    wide = smooth(48, 128, 3, 90)
    c["right_half"] = window(wide, 64, 64, quality=95, subsampling="420")
    c["right_half_odd_lead"] = window(wide, 64, 64, lead=1, quality=95, subsampling="444", restart=5)
    c["odd_window_odd_lead"] = window(wide, 31, 45, lead=3, quality=80, subsampling="420", restart=2)
    c["gray_odd_lead"] = window(smooth(30, 50, 1, 91), 8, 33, lead=5, quality=95)
    c["bgra_odd_lead"] = window(smooth(30, 50, 4, 92), 3, 41, lead=1, quality=95, subsampling="420", restart=3)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """(coefficients, block bits, file) of a case by the restatement"""
    c = shared_cases()[name]
    img = np.ascontiguousarray(c.image())
    g = R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart)
    zz = R.coefficients(img, c.quality, c.subsampling)
    return zz, R.block_bits(zz, g), R.encode(img, c.quality, c.subsampling, c.restart)


def intervals(name):
    """per interval of a case: (bits before the pad, the unstuffed bytes with the pad)"""
    c = shared_cases()[name]
    g = R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart)
    zz = reference(name)[0]
    blk, bits, length = R.tokens(zz, g)
    iv = (blk // g.bpm) // g.restart
    out = []
    for i in range(g.nint):
        m = iv == i
        n = int(length[m].sum())
        pad = -n % 8
        out.append((n, R._bytes_of(np.append(bits[m], (1 << pad) - 1), np.append(length[m], pad)).tobytes()))
    return out
