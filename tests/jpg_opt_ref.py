"""Restatement of the device JPEG encoder's optimised Huffman tables (``optimize=True``): the symbol
histograms of an image's coefficients, libjpeg's ``jpeg_gen_optimal_table`` procedure in plain Python, the file with the built DHT.

Builds on jpg_ref.py, which it leaves as it is: the coefficients, the DC differences, the token coder, the scan and the other header
segments are that module's.  The token coder reads its code tables from two module attributes; ``scan`` here lends it the built
tables for the length of one call.  Exact integer arithmetic: the product's host build (tests/host_jpeg_opt/jpeg_opt_emul.hip) and its
kernels (csrc/kernels_jpeg_opt.hip) are held to these bytes with 0 differing.
"""
from __future__ import annotations

import contextlib
import struct

import numpy as np

import jpg_ref as R

TABLE_IDS = [0x00, 0x10, 0x01, 0x11]  # DC luminance, AC luminance, DC chrominance, AC chrominance: the DHT segment's order


# ---- the symbols -----------------------------------------------------------------------------------------------------------------------
def histograms(zz, g):
    """the counts of the symbols the token coder emits, by table in the DHT's order: (4, 256) int64; the chrominance rows of a
    one-component image are zero.  DC: the category of every difference.  AC: a run / size symbol per non-zero coefficient, a ZRL
    (0xF0) per 16 zeros in front of one, and EOB (0) for a block whose last coefficient is zero."""
    n = len(zz)
    tab = np.minimum(np.tile(g.comp, g.nmcu), 1)
    h = np.zeros((4, 256), np.int64)
    np.add.at(h, (2 * tab, R._size(R.dc_differences(zz, g))), 1)
    blk, k = np.nonzero(zz[:, 1:])
    k = k + 1
    first = np.concatenate([[True], blk[1:] != blk[:-1]]) if len(blk) else np.zeros(0, bool)
    run = k - np.where(first, 0, np.concatenate([[0], k[:-1]])) - 1
    t = tab[blk]
    np.add.at(h, (2 * t + 1, ((run & 15) << 4) | R._size(zz[blk, k].astype(np.int64))), 1)
    np.add.at(h, (2 * t + 1, np.full(len(t), 0xF0)), run >> 4)
    last = np.zeros(n, np.int64)
    np.maximum.at(last, blk, k)
    np.add.at(h, (2 * tab[last < 63] + 1, 0), 1)
    return h


# ---- the table of a histogram ------------------------------------------------------------------------------------------------------------
def code_sizes(counts):
    """the code size of every symbol before the limit to 16 bits: 257 entries, the last the reserved symbol of frequency 1 (so that no
    real symbol gets the code of all ones).  The two least frequent non-zero entries are merged until one is left; among equals the
    scans, ascending with ``<=``, take the larger index; every symbol of either subtree grows by a bit."""
    freq = [int(c) for c in counts] + [0] * (256 - len(counts)) + [1]
    size, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, None
        for i in range(257):
            if freq[i] and (v is None or freq[i] <= v):
                v, c1 = freq[i], i
        c2, v = -1, None
        for i in range(257):
            if freq[i] and i != c1 and (v is None or freq[i] <= v):
                v, c2 = freq[i], i
        if c2 < 0:
            return size
        freq[c1] += freq[c2]
        freq[c2] = 0
        size[c1] += 1
        while others[c1] >= 0:  # the chain of the symbols of c1's subtree ...
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2         # ... continues with c2's
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1


def limit_bits(size):
    """BITS (index 1 ... 16) of code sizes: Annex K.2's adjustment (figure K.3) until no code is longer than 16 bits, then the
    reserved symbol's code point taken off the longest length"""
    bits = [0] * (max(max(size), 16) + 1)
    for s in size:
        if s:
            bits[s] += 1
    for i in range(len(bits) - 1, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    return bits[1:17]


def optimal_table(counts):
    """(BITS, HUFFVAL) of a histogram, as jpg_ref's table specs: HUFFVAL by code size, then by symbol"""
    size = code_sizes(counts)
    vals = [j for s in range(1, max(size) + 1) for j in range(256) if size[j] == s]
    return limit_bits(size), vals


def tables(zz, g):
    """the image's table specs in the DHT's order: two for one component, four for three"""
    h = histograms(zz, g)
    return [optimal_table(h[t]) for t in range(2 if g.nc == 1 else 4)]


# ---- the file ---------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _coder_tables(specs):
    """jpg_ref's token coder with these tables (DHT order) for the length of the block"""
    keep = R._DC, R._AC
    codes = [R.code_table(s) for s in specs]
    R._DC, R._AC = [codes[0], codes[2 % len(codes)]], [codes[1], codes[3 % len(codes)]]
    try:
        yield
    finally:
        R._DC, R._AC = keep


def scan(zz, g, specs):
    with _coder_tables(specs):
        return R.scan(zz, g)


def dht_body(specs):
    return b"".join(bytes([tc]) + bytes(s[0]) + bytes(s[1]) for tc, s in zip(TABLE_IDS, specs))


def headers(g, quality, specs):
    """jpg_ref.headers with the built tables in the DHT segment"""
    plain = R.headers(g, quality)
    std = [(0x00, R.DC_LUMA), (0x10, R.AC_LUMA)] + ([(0x01, R.DC_CHROMA), (0x11, R.AC_CHROMA)] if g.nc == 3 else [])
    old = R._segment(0xC4, b"".join(bytes([tc]) + bytes(s[0]) + bytes(s[1]) for tc, s in std))
    assert plain.count(old) == 1
    return plain.replace(old, R._segment(0xC4, dht_body(specs)))


def parts(img, quality=95, subsampling="420", restart_mcus=None):
    """(specs, header, scan) of the optimised file"""
    a = np.asarray(img)
    assert a.dtype == np.uint8
    a = a if a.ndim == 3 else a[..., None]
    g = R.Geom(a.shape[0], a.shape[1], a.shape[2], subsampling, restart_mcus)
    zz = R.coefficients(a, quality, subsampling)
    specs = tables(zz, g)
    return specs, headers(g, quality, specs), scan(zz, g, specs)


def encode(img, quality=95, subsampling="420", restart_mcus=None, optimize=True):
    """the whole file; ``optimize=False``: jpg_ref.encode"""
    if not optimize:
        return R.encode(img, quality, subsampling, restart_mcus)
    _, head, data = parts(img, quality, subsampling, restart_mcus)
    return head + data + b"\xff\xd9"


def dht_of(data):
    """the table specs of a file's DHT segment, in its order"""
    at = data.index(b"\xff\xc4")
    (n,) = struct.unpack(">H", data[at + 2:at + 4])
    body, out = data[at + 4:at + 2 + n], []
    while body:
        bits = list(body[1:17])
        out.append((body[0], bits, list(body[17:17 + sum(bits)])))
        body = body[17 + sum(bits):]
    return out
