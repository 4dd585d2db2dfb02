"""NumPy restatement of the device JPEG encoder's file: the contract in code.

Baseline sequential DCT, 8-bit, the Annex K quantisation tables scaled by the IJG quality rule, the Annex K Huffman tables, restart
intervals.  Exact integer arithmetic throughout, so the product's host build (tests/host_jpeg/jpeg_emul.hip) and its kernels
(csrc/kernels_jpeg.hip) are held to these bytes with 0 differing.  Vectorised over blocks and tokens so that whole frames can be
restated; ``encode_block_scalar`` states the entropy coder of one block the plain way and the host tests hold the two together.
"""
from __future__ import annotations

import struct

import numpy as np

SUBSAMPLINGS = {"444": 0, "420": 2}  # the ABI's codes (Pillow's numbering)

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])  # natural (row-major) index of zigzag position k

# ISO/IEC 10918-1 Annex K.1 / K.2, row-major
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80,
                   62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95,
                   98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
                     99, 99] + [99] * 32)

# Annex K.3 - K.6: the number of codes of each length 1 ... 16, and the symbols in code order
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1,
    0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA,
    0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
    0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
    0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19,
    0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8,
    0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4,
    0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
    0xFA])

MAX_BLOCK_BITS = 22 + 63 * 26  # the longest DC token (chrominance, category 11) and 63 times the longest AC token: what no block exceeds


def _rng(seed):
    return np.random.default_rng(seed)


def code_table(spec, size=256):
    """(codes, lengths) by symbol of a (BITS, HUFFVAL) table: canonical codes, Annex C"""
    bits, vals = spec
    code = np.zeros(size, np.int64)
    length = np.zeros(size, np.int64)
    c, k = 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            code[vals[k]], length[vals[k]] = c, n
            c, k = c + 1, k + 1
        c <<= 1
    return code, length


_DC = [code_table(DC_LUMA), code_table(DC_CHROMA)]
_AC = [code_table(AC_LUMA), code_table(AC_CHROMA)]


def quant_table(base, quality):
    """the IJG quality rule, row-major"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality must be 1 ... 100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((base * s + 50) // 100, 1, 255)


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
class Geom:
    def __init__(self, h, w, cn, subsampling="420", restart_mcus=None):
        if subsampling not in SUBSAMPLINGS:
            raise ValueError(f"subsampling must be one of {sorted(SUBSAMPLINGS)}")
        if cn not in (1, 3, 4) or not (1 <= h <= 65535 and 1 <= w <= 65535):
            raise ValueError("outside what the encoder takes")
        self.h, self.w, self.cn = h, w, cn
        self.nc = 1 if cn == 1 else 3
        self.sub = self.nc == 3 and subsampling == "420"
        self.m = 16 if self.sub else 8                       # MCU edge
        self.bpm = 1 if self.nc == 1 else 6 if self.sub else 3  # blocks per MCU
        self.mcux, self.mcuy = -(-w // self.m), -(-h // self.m)
        self.nmcu = self.mcux * self.mcuy
        self.restart = default_restart_mcus(h, w, cn, subsampling) if restart_mcus is None else int(restart_mcus)
        if not 1 <= self.restart <= 65535:
            raise ValueError("restart_mcus must be 1 ... 65535")
        self.nint = -(-self.nmcu // self.restart)
        self.nblocks = self.nmcu * self.bpm
        # component of each block of an MCU
        self.comp = np.array([0] if self.nc == 1 else [0, 0, 0, 0, 1, 2] if self.sub else [0, 1, 2])


def default_restart_mcus(h, w, cn, subsampling="420"):
    """one MCU row per interval, capped at the field's 65535 (the widest image has 8192 MCUs per row, so the cap never binds):
    an 8192 x 4096 frame gets 256 intervals in 4:2:0 and 512 in 4:4:4"""
    m = 16 if (cn != 1 and subsampling == "420") else 8
    return min(65535, -(-w // m))


def bound(h, w, cn, subsampling="420", restart_mcus=None):
    """bytes the scan can need: every block at MAX_BLOCK_BITS, every byte stuffed, one pad byte and one marker per interval"""
    g = Geom(h, w, cn, subsampling, restart_mcus)
    return 2 * (g.nblocks * ((MAX_BLOCK_BITS + 7) // 8) + g.nint) + 2 * g.nint


# ---- pixels to coefficients -----------------------------------------------------------------------------------------------------------
def planes(img, subsampling="420"):
    """the component planes, padded to whole MCUs by repeating the last column and row (before downsampling)"""
    a = img if img.ndim == 3 else img[..., None]
    h, w, cn = a.shape
    g = Geom(h, w, cn, subsampling, 1)
    a = np.pad(a[..., :3] if cn == 4 else a, ((0, g.mcuy * g.m - h), (0, g.mcux * g.m - w), (0, 0)), mode="edge").astype(np.int64)
    if cn == 1:
        return [a[..., 0]]
    b, gr, r = a[..., 0], a[..., 1], a[..., 2]
    y = (19595 * r + 38470 * gr + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * gr + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * gr - 5329 * b + (128 << 16) + 32767) >> 16
    if g.sub:
        cb, cr = [(p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2 for p in (cb, cr)]
    return [y, cb, cr]


def _blocks_of(p, mcuy, mcux, n):
    """(mcuy, mcux, n * n, 8, 8): the n x n blocks of every MCU of one plane, raster order inside the MCU"""
    return p.reshape(mcuy, n, 8, mcux, n, 8).transpose(0, 3, 1, 4, 2, 5).reshape(mcuy, mcux, n * n, 8, 8)


def sample_blocks(img, subsampling="420"):
    """(nblocks, 8, 8) level-shifted samples, MCU-major: per MCU its Y block(s), then Cb, then Cr"""
    a = img if img.ndim == 3 else img[..., None]
    g = Geom(a.shape[0], a.shape[1], a.shape[2], subsampling, 1)
    ps = planes(a, subsampling)
    parts = [_blocks_of(ps[0], g.mcuy, g.mcux, 2 if g.sub else 1)] + [_blocks_of(p, g.mcuy, g.mcux, 1) for p in ps[1:]]
    return np.concatenate(parts, axis=2).reshape(-1, 8, 8) - 128


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """one pass of the IJG "islow" forward DCT along the last axis: 13-bit constants; the first pass leaves two extra bits, the second
    removes them, and the whole transform is scaled by 8"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[0], out[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    n = 11 if first else 15
    z1 = (t12 + t13) * 4433
    out[2], out[6] = _descale(z1 + t13 * 6270, n), _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[7], out[5], out[3], out[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def fdct(blocks):
    """(n, 8, 8) samples -> (n, 8, 8) DCT outputs times 8: rows first, then columns"""
    rows = _fdct_pass(blocks.astype(np.int64), True)
    return _fdct_pass(rows.transpose(0, 2, 1), False).transpose(0, 2, 1)


def coefficients(img, quality=95, subsampling="420"):
    """(nblocks, 64) int16 quantised coefficients in zigzag order, MCU-major"""
    a = img if img.ndim == 3 else img[..., None]
    g = Geom(a.shape[0], a.shape[1], a.shape[2], subsampling, 1)
    d = fdct(sample_blocks(a, subsampling)).reshape(-1, 64)
    q = np.stack([quant_table(Q_LUMA, quality), quant_table(Q_CHROMA, quality)])[np.minimum(g.comp, 1)]  # (bpm, 64)
    q8 = 8 * np.tile(q, (g.nmcu, 1))
    c = np.sign(d) * ((np.abs(d) + q8 // 2) // q8)  # rounded half away from zero
    return c[:, ZIGZAG].astype(np.int16)


# ---- entropy coding -------------------------------------------------------------------------------------------------------------------
def _size(v):
    """the category of a value: the bits of its magnitude"""
    return np.frexp(np.abs(v).astype(np.float64))[1].astype(np.int64)  # (exact: the exponent of m * 2 ** e with 0.5 <= m < 1)


def _amp(v, s):
    """the s amplitude bits of v: v itself if positive, else v - 1 in s bits"""
    return np.where(v >= 0, v, v + (1 << s) - 1).astype(np.int64)


def dc_differences(zz, g):
    """the DC difference of every block: against the previous block of its component, 0 at the start of every interval"""
    n = len(zz)
    comp = np.tile(g.comp, g.nmcu)
    interval = (np.arange(n) // g.bpm) // g.restart
    diff = np.zeros(n, np.int64)
    for c in range(g.nc):
        idx = np.nonzero(comp == c)[0]
        dc = zz[idx, 0].astype(np.int64)
        prev = np.concatenate([[0], dc[:-1]])
        prev[np.concatenate([[True], interval[idx][1:] != interval[idx][:-1]])] = 0
        diff[idx] = dc - prev
    return diff


def tokens(zz, g):
    """every token of the scan in order: (block, bits, length) with bits < 2 ** length.  One token per block for the DC difference,
    one per non-zero AC coefficient (its ZRLs in front of it, run / size code, amplitude) and one EOB where a block's last
    coefficient is zero."""
    n = len(zz)
    tab = np.minimum(np.tile(g.comp, g.nmcu), 1)
    diff = dc_differences(zz, g)
    s = _size(diff)
    dcc, dcl = np.stack([t[0] for t in _DC]), np.stack([t[1] for t in _DC])
    acc, acl = np.stack([t[0] for t in _AC]), np.stack([t[1] for t in _AC])
    dc_bits = (dcc[tab, s] << s) | _amp(diff, s)
    dc_len = dcl[tab, s] + s
    blk, k = np.nonzero(zz[:, 1:])
    k = k + 1
    v = zz[blk, k].astype(np.int64)
    first = np.concatenate([[True], blk[1:] != blk[:-1]]) if len(blk) else np.zeros(0, bool)
    prev = np.where(first, 0, np.concatenate([[0], k[:-1]]))
    run = k - prev - 1
    s = _size(v)
    t = tab[blk]
    rs = ((run & 15) << 4) | s
    zrl = run >> 4                                      # 0 ... 3 ZRL codes (0xF0) in front
    zc, zl = acc[t, 0xF0], acl[t, 0xF0]
    ac_bits, ac_len = np.zeros(len(v), np.int64), np.zeros(len(v), np.int64)
    for i in range(3):
        m = zrl > i
        ac_bits, ac_len = np.where(m, (ac_bits << zl) | zc, ac_bits), np.where(m, ac_len + zl, ac_len)
    ac_bits = (((ac_bits << acl[t, rs]) | acc[t, rs]) << s) | _amp(v, s)
    ac_len = ac_len + acl[t, rs] + s
    last = np.zeros(n, np.int64)
    np.maximum.at(last, blk, k)
    eob = np.nonzero(last < 63)[0]
    te = tab[eob]
    key = np.concatenate([np.arange(n) * 66, blk * 66 + k, eob * 66 + 64])
    order = np.argsort(key, kind="stable")
    return (np.concatenate([np.arange(n), blk, eob])[order], np.concatenate([dc_bits, ac_bits, acc[te, 0]])[order],
            np.concatenate([dc_len, ac_len, acl[te, 0]])[order])


def block_bits(zz, g):
    """the coded bits of every block"""
    blk, _, length = tokens(zz, g)
    return np.bincount(blk, weights=length, minlength=len(zz)).astype(np.int64)


def _bytes_of(bits, length):
    """the bytes of tokens laid most significant bit first; the total length is a multiple of 8"""
    out = []
    edges = np.concatenate([[0], np.cumsum(length)])
    i0 = 0
    while i0 < len(length):
        i1 = int(np.searchsorted(edges, edges[i0] + (1 << 25), side="right")) - 1  # about 4 MB of stream per round
        i1 = max(i1, i0 + 1)
        i1 = min(i1, len(length))
        ln, bt = length[i0:i1], bits[i0:i1]
        tok = np.repeat(np.arange(len(ln)), ln)
        j = np.arange(int(ln.sum())) - np.repeat(edges[i0:i1] - edges[i0], ln)
        out.append(((bt[tok] >> (ln[tok] - 1 - j)) & 1).astype(np.uint8))
        i0 = i1
    flat = np.concatenate(out) if out else np.zeros(0, np.uint8)
    assert len(flat) % 8 == 0
    return np.packbits(flat)


def scan(zz, g):
    """the entropy-coded data with its markers: every interval padded with 1-bits to a whole byte, 0x00 behind every 0xFF data byte,
    RSTm (m = k mod 8) behind every interval k but the last"""
    blk, bits, length = tokens(zz, g)
    interval = (blk // g.bpm) // g.restart
    ibits = np.bincount(interval, weights=length, minlength=g.nint).astype(np.int64)
    pad = (-ibits) % 8
    # the pad of every interval as one more token behind its last
    key = np.concatenate([np.arange(len(blk)) * 2, (np.cumsum(np.bincount(interval, minlength=g.nint)) - 1) * 2 + 1])
    order = np.argsort(key, kind="stable")
    bits = np.concatenate([bits, (1 << pad) - 1])[order]
    length = np.concatenate([length, pad])[order]
    raw = _bytes_of(bits, length)
    ends = np.cumsum((ibits + pad) // 8)                 # unstuffed bytes up to the end of every interval
    ff = np.nonzero(raw == 0xFF)[0]
    stuffed = np.insert(raw, ff + 1, 0)
    ends = ends + np.searchsorted(ff, ends, side="left")  # ... and stuffed
    at = np.repeat(ends[:-1], 2)
    marks = np.stack([np.full(g.nint - 1, 0xFF), 0xD0 + np.arange(g.nint - 1) % 8], axis=1).reshape(-1).astype(np.uint8)
    return np.insert(stuffed, at, marks).tobytes()


def encode_block_scalar(zz, pred, tab):
    """one block the plain way: [(bits, length), ...] of its DC difference against ``pred`` and its AC coefficients"""
    out = []
    d = int(zz[0]) - pred
    s = abs(d).bit_length()
    out.append((int(_DC[tab][0][s]) << s | (d if d >= 0 else d + (1 << s) - 1), int(_DC[tab][1][s]) + s))
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((int(_AC[tab][0][0xF0]), int(_AC[tab][1][0xF0])))
            run -= 16
        s = abs(v).bit_length()
        rs = run << 4 | s
        out.append((int(_AC[tab][0][rs]) << s | (v if v >= 0 else v + (1 << s) - 1), int(_AC[tab][1][rs]) + s))
        run = 0
    if run:
        out.append((int(_AC[tab][0][0]), int(_AC[tab][1][0])))
    return out


# ---- the file -------------------------------------------------------------------------------------------------------------------------
def _segment(marker, body):
    return struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body


def headers(g, quality):
    """SOI, APP0 (JFIF 1.01, aspect 1:1), DQT, SOF0, DHT, DRI, SOS"""
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    tables = [Q_LUMA] if g.nc == 1 else [Q_LUMA, Q_CHROMA]
    out += _segment(0xDB, b"".join(bytes([i]) + bytes(quant_table(t, quality)[ZIGZAG].tolist()) for i, t in enumerate(tables)))
    samp = 0x22 if g.sub else 0x11
    comps = b"".join(bytes([i + 1, samp if i == 0 else 0x11, min(i, 1)]) for i in range(g.nc))
    out += _segment(0xC0, struct.pack(">BHHB", 8, g.h, g.w, g.nc) + comps)
    specs = [(0x00, DC_LUMA), (0x10, AC_LUMA)] + ([(0x01, DC_CHROMA), (0x11, AC_CHROMA)] if g.nc == 3 else [])
    out += _segment(0xC4, b"".join(bytes([tc]) + bytes(s[0]) + bytes(s[1]) for tc, s in specs))
    out += _segment(0xDD, struct.pack(">H", g.restart))
    sel = b"".join(bytes([i + 1, 0x11 * min(i, 1)]) for i in range(g.nc))
    return out + _segment(0xDA, bytes([g.nc]) + sel + b"\x00\x3f\x00")


def encode(img, quality=95, subsampling="420", restart_mcus=None):
    """the whole file of a uint8 (H, W[, C]) image in cv2 channel order (C 1, 3 or 4; alpha is dropped)"""
    a = np.asarray(img)
    assert a.dtype == np.uint8
    a = a if a.ndim == 3 else a[..., None]
    g = Geom(a.shape[0], a.shape[1], a.shape[2], subsampling, restart_mcus)
    return headers(g, quality) + scan(coefficients(a, quality, subsampling), g) + b"\xff\xd9"


def decode(data):
    """Pillow's decoding of a file, in cv2 channel order"""
    import io

    from PIL import Image

    im = Image.open(io.BytesIO(data))
    a = np.asarray(im)
    return a if a.ndim == 2 else np.ascontiguousarray(a[..., ::-1])
