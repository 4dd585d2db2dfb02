"""NumPy restatement of the device PNG encoder's stream: what ``encode_png_tensor`` must return, byte
for byte.  Written from the contract, not from the kernels: whole-band array operations, the RFC 1951 tables typed in from the RFC,
the container and its CRC made with zlib.

* scanlines: filter byte, then the samples in PNG order (gray / RGB / RGBA, 16-bit big-endian); filter 2 (Up) or 4 (Paeth) on every
  row, predicted from the unfiltered image (the row above a band's first row is the image's, zero only above row 0);
* bands of ``band_rows`` rows; a band's scanline bytes are cut into segments of SEG = 256 bytes counted from the band's start;
* tokens: inside a segment, a maximal run of L bytes equal to the byte before them is one match (distance 1, length L) if
  L >= MIN_MATCH = 4 and L literals otherwise; every other byte is a literal;
* one dynamic Huffman block per band (``code_lengths`` below, limit 15; the code lengths sent without run-length symbols through a
  code-length code of limit 7; one distance code of one bit), end of block, an empty stored block padding to a byte; a band that would
  be larger than its stored form (5 bytes per started 65535) goes out as stored blocks;
* the zlib stream: 78 01, the bands, one empty final stored block, Adler-32; the container: IHDR, vrBD, one IDAT, IEND.
"""
from __future__ import annotations

import io
import struct
import zlib

import numpy as np

SEG, MIN_MATCH = 256, 4
STORED_MAX = 65535
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FILTERS = {"up": 2, "paeth": 4}

# RFC 1951 3.2.5: (symbol, extra bits, first length)
_LEN_ROWS = [(257, 0, 3), (258, 0, 4), (259, 0, 5), (260, 0, 6), (261, 0, 7), (262, 0, 8), (263, 0, 9), (264, 0, 10), (265, 1, 11),
             (266, 1, 13), (267, 1, 15), (268, 1, 17), (269, 2, 19), (270, 2, 23), (271, 2, 27), (272, 2, 31), (273, 3, 35), (274, 3, 43),
             (275, 3, 51), (276, 3, 59), (277, 4, 67), (278, 4, 83), (279, 4, 99), (280, 4, 115), (281, 5, 131), (282, 5, 163),
             (283, 5, 195), (284, 5, 227), (285, 0, 258)]
LEN_SYM = np.zeros(259, np.int64)
LEN_XBITS = np.zeros(259, np.int64)
LEN_XVAL = np.zeros(259, np.int64)
for _sym, _xb, _base in _LEN_ROWS:
    for _v in range(_base, min(_base + (1 << _xb), 259)):
        if _sym == 284 and _v == 258:
            continue
        LEN_SYM[_v], LEN_XBITS[_v], LEN_XVAL[_v] = _sym, _xb, _v - _base
SYM_XBITS = np.zeros(286, np.int64)
for _sym, _xb, _base in _LEN_ROWS:
    SYM_XBITS[_sym] = _xb


# ---- scanlines ----------------------------------------------------------------------------------------------------------------------
def png_order(img: np.ndarray) -> np.ndarray:
    """(H, W, C) cv2 order -> (H, W * C * itemsize) bytes in PNG order"""
    a = img if img.ndim == 3 else img[..., None]
    cn = a.shape[2]
    if cn >= 3:
        a = a[..., [2, 1, 0] + ([3] if cn == 4 else [])]
    if a.dtype == np.uint16:
        a = a.astype(">u2")
    return np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)


def scanlines(img: np.ndarray, filter: str = "up") -> np.ndarray:
    raw = png_order(img).astype(np.int16)
    a = img if img.ndim == 3 else img[..., None]
    bpp = a.shape[2] * a.dtype.itemsize
    up = np.zeros_like(raw)
    up[1:] = raw[:-1]
    if filter == "up":
        pred = up
    else:
        left = np.zeros_like(raw)
        left[:, bpp:] = raw[:, :-bpp]
        ul = np.zeros_like(raw)
        ul[:, bpp:] = up[:, :-bpp]
        p = left + up - ul
        pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
        pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    out = np.empty((raw.shape[0], raw.shape[1] + 1), np.uint8)
    out[:, 0] = FILTERS[filter]
    out[:, 1:] = (raw - pred).astype(np.uint8)
    return out


# ---- codes --------------------------------------------------------------------------------------------------------------------------
def package_merge(freq, limit: int) -> np.ndarray:
    """optimal length-limited lengths, the plain way: the reference the two-stage rule of ``code_lengths`` falls back to"""
    freq = [int(f) for f in freq]
    used = sorted((s for s in range(len(freq)) if freq[s]), key=lambda s: (freq[s], s))
    m = len(used)
    prev: list[tuple[int, int]] = []  # (weight, counts of the leaves, 4 bits each)
    for _ in range(limit):
        pk = [(prev[i][0] + prev[i + 1][0], prev[i][1] + prev[i + 1][1]) for i in range(0, len(prev) - 1, 2)]
        cur, a, b = [], 0, 0
        while a < m or b < len(pk):
            if b >= len(pk) or (a < m and freq[used[a]] <= pk[b][0]):
                cur.append((freq[used[a]], 1 << (4 * a)))
                a += 1
            else:
                cur.append(pk[b])
                b += 1
        prev = cur
    total = sum(c for _, c in prev[:2 * m - 2])
    out = np.zeros(len(freq), np.int64)
    for k, s in enumerate(used):
        out[s] = (total >> (4 * k)) & 15
    return out


def code_lengths(freq, limit: int = 15) -> np.ndarray:
    """The stated rule: symbols sorted by (count, symbol); the two-queue Huffman tree (the lighter front of the leaf queue and the
    package queue, the leaf on a tie); if a leaf is deeper than ``limit``, package-merge instead.  Fewer than two used symbols: one
    bit for the used one (symbol 0 if none) and one for the lowest other symbol."""
    freq = [int(f) for f in freq]
    out = np.zeros(len(freq), np.int64)
    used = sorted((s for s in range(len(freq)) if freq[s]), key=lambda s: (freq[s], s))
    if len(used) < 2:
        a = used[0] if used else 0
        out[a] = 1
        out[1 if a == 0 else 0] = 1
        return out
    m = len(used)
    w = [freq[s] for s in used]
    parent = [0] * (2 * m - 1)
    a, b = 0, m
    while len(w) < 2 * m - 1:
        pick = []
        for _ in range(2):
            if b >= len(w) or (a < m and w[a] <= w[b]):
                pick.append(a)
                a += 1
            else:
                pick.append(b)
                b += 1
        parent[pick[0]] = parent[pick[1]] = len(w)
        w.append(w[pick[0]] + w[pick[1]])
    depth = [0] * (2 * m - 1)
    for i in range(2 * m - 3, -1, -1):
        depth[i] = depth[parent[i]] + 1
    if max(depth[:m]) > limit:
        return package_merge(freq, limit)
    for k, s in enumerate(used):
        out[s] = depth[k]
    return out


def canonical(lengths) -> np.ndarray:
    """bit-reversed canonical codes (RFC 1951 3.2.2)"""
    lengths = np.asarray(lengths, np.int64)
    out = np.zeros(len(lengths), np.int64)
    code = 0
    for n in range(1, 16):
        for s in np.flatnonzero(lengths == n):
            out[s] = int(format(code, f"0{n}b")[::-1], 2)
            code += 1
        code <<= 1
    return out


# ---- one band -----------------------------------------------------------------------------------------------------------------------
def tokens(s: np.ndarray):
    """positions, kinds (1 literal, 2 match) and lengths of the tokens of a band's scanline bytes"""
    n = s.size
    eq = np.zeros(n + 2, np.int8)
    eq[2:n + 1] = s[1:] == s[:-1]
    eq[1:n + 1][np.arange(n) % SEG == 0] = 0
    d = np.diff(eq)
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    long = ends - starts >= MIN_MATCH
    starts, ends = starts[long], ends[long]
    cover = np.zeros(n + 1, np.int64)
    np.add.at(cover, starts, 1)
    np.add.at(cover, ends, -1)
    kind = np.where(np.cumsum(cover)[:n] > 0, 0, 1)
    kind[starts] = 2
    length = np.zeros(n, np.int64)
    length[starts] = ends - starts
    pos = np.flatnonzero(kind)
    return pos, kind[pos], length[pos]


def _pack(nbytes: int, offsets: np.ndarray, values: np.ndarray) -> np.ndarray:
    """bytes with `values` ORed in at bit `offsets` (the fields are disjoint, so a sum is the OR)"""
    x = values.astype(np.uint64) << (offsets & 7).astype(np.uint64)
    acc = np.zeros(nbytes + 8, np.float64)
    for k in range(5):
        acc += np.bincount((offsets >> 3) + k, weights=((x >> np.uint64(8 * k)) & np.uint64(255)).astype(np.float64), minlength=nbytes + 8)
    return acc[:nbytes].astype(np.uint8)


def stored_band(s: np.ndarray) -> bytes:
    out = b""
    for o in range(0, s.size, STORED_MAX):
        part = s[o:o + STORED_MAX].tobytes()
        out += b"\x00" + struct.pack("<HH", len(part), 65535 - len(part)) + part
    return out


def band(s: np.ndarray) -> tuple[bytes, bool]:
    """a band's segment of the stream and whether it is stored"""
    pos, kind, length = tokens(s)
    lit = kind == 1
    sym = np.where(lit, s[pos].astype(np.int64), LEN_SYM[length])
    freq = np.bincount(sym, minlength=286)
    freq[256] = 1
    L = code_lengths(freq, 15)
    codes = canonical(L)
    hlit = max(257, int(np.flatnonzero(L).max()) + 1)
    sent = np.concatenate([L[:hlit], [1]])
    CL = code_lengths(np.bincount(sent, minlength=19), 7)
    clc = canonical(CL)
    order_len = [int(CL[o]) for o in CL_ORDER]
    hclen = max(4, max(i for i, v in enumerate(order_len) if v) + 1)
    fields = [(0, 1), (2, 2), (hlit - 257, 5), (0, 5), (hclen - 4, 4)] + [(v, 3) for v in order_len[:hclen]]
    fields += [(int(clc[v]), int(CL[v])) for v in sent]
    hv = np.array([f[0] for f in fields], np.int64)
    hn = np.array([f[1] for f in fields], np.int64)
    xb = np.where(lit, 0, LEN_XBITS[length])
    tn = L[sym] + xb + np.where(lit, 0, 1)
    tv = codes[sym] | np.where(lit, 0, LEN_XVAL[length] << L[sym])
    vals = np.concatenate([hv, tv, [codes[256]]])
    nbits = np.concatenate([hn, tn, [L[256]]])
    offs = np.concatenate([[0], np.cumsum(nbits)])
    total = int(offs[-1]) + 3
    body = (total + 7) // 8
    stored = stored_band(s)
    if body + 4 > len(stored):
        return stored, True
    out = _pack(body, offs[:-1], vals).tobytes() + b"\x00\x00\xff\xff"
    return out, False


# ---- the file -----------------------------------------------------------------------------------------------------------------------
def bound(h: int, w: int, cn: int, itemsize: int, band_rows: int) -> int:
    stride = 1 + w * cn * itemsize
    rows = min(band_rows, h)
    total = 0
    for r in range(0, h, rows):
        n = (min(r + rows, h) - r) * stride
        total += n + 5 * (-(-n // STORED_MAX)) + 8
    return total


def deflate(img: np.ndarray, *, filter: str = "up", band_rows: int = 8):
    """(segments, bands): the concatenated band segments and per band (row0, row1, offset, size, adler32, stored)"""
    lines = scanlines(img, filter)
    h = lines.shape[0]
    rows = min(band_rows, h)
    parts, bands, off = [], [], 0
    for r in range(0, h, rows):
        s = lines[r:r + rows].reshape(-1)
        p, st = band(s)
        bands.append((r, min(r + rows, h), off, len(p), zlib.adler32(s.tobytes()) & 0xFFFFFFFF, int(st)))
        parts.append(p)
        off += len(p)
    return b"".join(parts), bands


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode(img: np.ndarray, *, filter: str = "up", band_rows: int = 8) -> bytes:
    a = img if img.ndim == 3 else img[..., None]
    h, w, cn = a.shape
    segs, bands = deflate(a, filter=filter, band_rows=band_rows)
    adler = zlib.adler32(scanlines(a, filter).tobytes()) & 0xFFFFFFFF
    stream = b"\x78\x01" + segs + b"\x01\x00\x00\xff\xff" + struct.pack(">I", adler)
    index = struct.pack(">BBI", 1, FILTERS[filter], len(bands))
    for r0, r1, off, _, _, _ in bands:
        index += struct.pack(">III", r0, r1, 2 + off)
    ihdr = struct.pack(">IIBBBBB", w, h, 8 * a.dtype.itemsize, {1: 0, 3: 2, 4: 6}[cn], 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"vrBD", index) + _chunk(b"IDAT", stream) + _chunk(b"IEND", b"")


# ---- a plain decoder for what Pillow and _png.decode do not take (16-bit) ---------------------------------------------------------
def decode(png: bytes) -> np.ndarray:
    """inflate + un-filter (types 0, 2, 4) of a non-interlaced PNG, back to cv2 channel order"""
    pos, idat, ihdr = 8, b"", None
    while pos < len(png):
        (n,), kind = struct.unpack(">I", png[pos:pos + 4]), png[pos + 4:pos + 8]
        body = png[pos + 8:pos + 8 + n]
        assert zlib.crc32(kind + body) & 0xFFFFFFFF == struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])[0], kind
        if kind == b"IHDR":
            ihdr = body
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, ct, _, _, _ = struct.unpack(">IIBBBBB", ihdr)
    cn, nb = {0: 1, 2: 3, 6: 4}[ct], depth // 8
    bpp = cn * nb
    lines = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * bpp)
    raw = np.zeros((h + 1, w * bpp + bpp), np.int64)  # a zero row above and a zero pixel to the left
    for r in range(h):
        f, cur = int(lines[r, 0]), lines[r, 1:].astype(np.int64)
        if f == 0:
            raw[r + 1, bpp:] = cur
        elif f == 2:
            raw[r + 1, bpp:] = (cur + raw[r, bpp:]) & 255
        else:
            assert f == 4, f
            for x in range(w * bpp):
                a, b, c = raw[r + 1, x], raw[r, x + bpp], raw[r, x]
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                raw[r + 1, x + bpp] = (cur[x] + (a if pa <= pb and pa <= pc else b if pb <= pc else c)) & 255
    body = raw[1:, bpp:].astype(np.uint8)
    img = (body.view(">u2").astype(np.uint16) if nb == 2 else body).reshape(h, w, cn)
    if cn >= 3:
        img = img[..., [2, 1, 0] + ([3] if cn == 4 else [])]
    return np.ascontiguousarray(img)


# ---- what the host and the GPU tests share ------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


def _half_noise():
    """noise in the top half, zero below: stored and coded bands in one file"""
    a = _rng(1).integers(0, 256, (64, 100, 3), dtype=np.uint8)
    a[32:] = 0
    return a


def _wide16(a):
    """a uint16 image with both bytes of every sample in use"""
    return (a.astype(np.uint16) << 8) | np.roll(a, 1, axis=1)


def cases() -> dict:
    """name -> (image, band_rows): the shape / type matrix the host and the GPU tests run, both filters over all of it"""
    import sphere_scene
    from vr180_convert_amd import synth

    return {
        "noise_disc": (synth.noise_disc(128, 128), 8),
        "pattern_200x131": (synth.pattern(131, 200), 8),                    # row bytes 600 + 1, height not a multiple of the band
        "sphere_256": (sphere_scene.render(256), 8),
        "zero": (np.zeros((96, 128, 3), np.uint8), 8),
        "all_255": (np.full((40, 64, 3), 255, np.uint8), 16),
        "noise_full": (_rng(2).integers(0, 256, (77, 96, 3), dtype=np.uint8), 8),      # every band stored
        "half_noise": (_half_noise(), 8),                                   # stored and coded bands in one file
        "one_pixel": (np.full((1, 1, 1), 7, np.uint8), 8),
        "gray_33x9": (_rng(3).integers(0, 256, (9, 33, 1), dtype=np.uint8) // 64 * 64, 4),
        "bgra_33x9": (_rng(4).integers(0, 4, (9, 33, 4), dtype=np.uint8), 2),          # row bytes 132 + 1
        "gray_width_7": (_rng(5).integers(0, 3, (50, 7, 1), dtype=np.uint8), 5),
        "noise_big_band": (_rng(6).integers(0, 256, (60, 500, 3), dtype=np.uint8), 50),  # 75 050 bytes per band: two stored blocks
        "zero_big_band": (np.zeros((130, 300, 3), np.uint8), 100),
        "gray16": (_wide16(synth.pattern(40, 52)[..., :1]), 8),
        "bgr16": (_wide16(sphere_scene.render(64)), 8),
        "bgra16_noise": (_rng(7).integers(0, 65536, (20, 31, 4), dtype=np.uint16), 8),
        "bgra16_flat": (np.full((20, 31, 4), 0x1234, np.uint16), 3),
    }


def _pil(png):
    from PIL import Image

    with Image.open(io.BytesIO(png)) as im:
        return np.asarray(im)


def _to_pil_order(img):
    cn = img.shape[2]
    return img[..., 0] if cn == 1 else img[..., ::-1] if cn == 3 else img[..., [2, 1, 0, 3]]


def check_file(png, img, filter, band_rows):
    """every reader the contract names returns the input pixels; the stream is one valid zlib stream and its bands inflate on their own"""
    from vr180_convert_amd import _png

    a = img if img.ndim == 3 else img[..., None]
    lines = scanlines(a, filter)
    pos = png.index(b"IDAT")
    (n,) = struct.unpack(">I", png[pos - 4:pos])
    stream = png[pos + 4:pos + 4 + n]
    assert zlib.decompress(stream) == lines.tobytes()  # (zlib checks the Adler-32)
    ipos = png.index(b"vrBD")
    version, ftype, nb = struct.unpack(">BBI", png[ipos + 4:ipos + 10])
    assert (version, ftype) == (1, FILTERS[filter]) and nb == -(-a.shape[0] // min(band_rows, a.shape[0]))
    bands = [struct.unpack(">III", png[ipos + 10 + 12 * k:ipos + 22 + 12 * k]) for k in range(nb)]
    for k, (r0, r1, off) in enumerate(bands):
        stop = bands[k + 1][2] if k + 1 < nb else len(stream) - 4
        d = zlib.decompressobj(-15)
        assert d.decompress(stream[off:stop]) == lines[r0:r1].tobytes(), k
    assert np.array_equal(decode(png), a)
    if a.dtype == np.uint8:
        assert np.array_equal(_pil(png), _to_pil_order(a))
        own = _png.decode(png)
        if filter == "up":
            assert own is not None and np.array_equal(own.reshape(a.shape), a)
        else:
            assert own is None  # the parallel reader declines Paeth: Pillow serves
