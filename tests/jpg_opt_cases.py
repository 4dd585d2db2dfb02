"""The images the optimised Huffman tables of the device JPEG encoder are held to, shared by the host half
(tests/test_jpeg_opt_host.py: the product's symbol walk and table builder on the CPU) and the GPU half (tests/test_gpu_jpeg_opt.py: the
kernels): the smallest shapes at which each part can still go wrong.  The restatement of each is computed once and shared."""
from __future__ import annotations

import functools
from pathlib import Path

import numpy as np

import jpg_cases as PC
import jpg_opt_ref as O
import jpg_ref as R

ROOT = Path(__file__).resolve().parents[1]
FLAT = "flat_8x8_gray"  # the one case whose scan cannot shrink: one byte either way


@functools.lru_cache(maxsize=None)
def docs_crop():
    """the 512 x 512 crop of the docs image whose luminance AC codes pass 16 bits before the limit"""
    from PIL import Image

    a = np.asarray(Image.open(ROOT / "tests" / "golden" / "ref_docs" / "test.jpg").convert("RGB"))
    return np.ascontiguousarray(a[512:1024, 512:1024, ::-1])


def corner(h, w, value, patch, seed):
    """a flat frame with a patch of noise in its corner: highly skewed counts"""
    a = np.full((h, w, 3), value, np.uint8)
    a[:patch, :patch] = PC.noise(patch, patch, 3, seed)
    return a


@functools.lru_cache(maxsize=None)
def shared_cases() -> dict:
    c = {}
    c[FLAT] = PC.dense(np.full((8, 8), 128, np.uint8), 95)                      # one DC symbol and EOB: one-bit codes
    c["noise_16x16_420"] = PC.dense(PC.noise(16, 16, 3, 200), 95, "420")         # one MCU, four tables
    c["restart1_17x9"] = PC.dense(PC.noise(17, 9, 3, 201) // 2 + PC.smooth(17, 9, 3, 202) // 2, 95, "420", 1)  # every interval starts at DC 0
    c["gray_136_q100"] = PC.dense(PC.noise(136, 136, 1, 203), 100)                 # 289 blocks: two workgroups of the histogram
    c["gray_136_q95_r1"] = PC.dense(PC.noise(136, 136, 1, 203), 95, restart=1)
    c["corner_420_q100"] = PC.dense(corner(256, 256, 120, 24, 204), 100, "420")
    c["corner_444_q100"] = PC.dense(corner(256, 256, 120, 24, 204), 100, "444")
    c["docs_420_q95"] = PC.dense(docs_crop(), 95, "420")                           # the limit to 16 bits acts
    c["docs_444_q95"] = PC.dense(docs_crop(), 95, "444")
    c["docs_444_q100"] = PC.dense(docs_crop(), 100, "444")
    c["bgra"] = PC.dense(PC.noise(20, 36, 4, 205) // 2 + PC.smooth(20, 36, 4, 206) // 2, 95, "420", 2)
    c["right_half"] = PC.window(PC.smooth(48, 128, 3, 207), 64, 64, quality=95, subsampling="420")  # one half of a side-by-side image
    return c


LIMITED = ("docs_420_q95", "docs_444_q95", "docs_444_q100")


@functools.lru_cache(maxsize=None)
def reference(name):
    """of a case by the restatements: (histograms, table specs, optimised file, standard-table file, code sizes before the limit)"""
    c = shared_cases()[name]
    img = np.ascontiguousarray(c.image())
    g = R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart)
    zz = R.coefficients(img, c.quality, c.subsampling)
    hist = O.histograms(zz, g)
    specs = O.tables(zz, g)
    data = O.headers(g, c.quality, specs) + O.scan(zz, g, specs) + b"\xff\xd9"
    sizes = [O.code_sizes(hist[t]) for t in range(len(specs))]
    return hist, specs, data, R.encode(img, c.quality, c.subsampling, c.restart), sizes


def scan_of(data):
    """the bytes between SOS's segment and EOI"""
    at = data.index(b"\xff\xda")
    return data[at + 2 + int.from_bytes(data[at + 2:at + 4], "big"):-2]
