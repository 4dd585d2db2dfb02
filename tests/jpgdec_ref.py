"""NumPy / plain Python restatement of the device JPEG decoder: the contract in code.

A file is parsed on the host (``parse``): the markers, the tables, the geometry, and one walk over the scan's 0xFF bytes that finds its
end and its RSTm markers.  The scan is unstuffed, cut into segments at the RSTm markers and tiled by subsequences of ``S`` bits
(``Stream``).  ``synchronise`` is the fixed-point iteration over the subsequences' entry states, ``sequential`` a plain decoder written
separately; the two must agree.  ``coefficients`` is the last pass, ``pixels`` the arithmetic behind it: dequantisation, libjpeg's
"islow" inverse DCT, its "fancy" chroma upsampling and its 16-bit YCbCr conversion.  The product's host build
(tests/host_jpegdec/jpegdec_emul.hip) and its kernels (csrc/kernels_jpegdec.hip) are held to these values with 0 differing.
"""
from __future__ import annotations

import numpy as np

from jpg_ref import ZIGZAG

DEFAULT_SUBSEQ_BITS = 1024


class Unsupported(Exception):
    """a valid file outside what the device decodes (V1C_E_UNSUPPORTED)"""


class Corrupt(Exception):
    """V1C_E_CORRUPT"""


def _at(e, pos):
    """the exception with the byte of the file the parse refuses it at (``pos``): what the product reports as error_pos"""
    e.pos = pos
    return e


# ---- the host-only parse ---------------------------------------------------------------------------------------------------------------
class Huff:
    """a DHT table: ``lut[first 16 bits] = length << 8 | symbol``, 0 where the bits start no code"""

    def __init__(self, bits, vals):
        self.bits, self.vals = list(bits), list(vals)
        lut = np.zeros(65536, np.int32)
        code, k = 0, 0
        for n in range(1, 17):
            if code + bits[n - 1] > 1 << n:
                raise Corrupt("DHT: more codes than the length holds")
            for _ in range(bits[n - 1]):
                lut[code << (16 - n):(code + 1) << (16 - n)] = n << 8 | vals[k]
                code, k = code + 1, k + 1
            code <<= 1
        self.lut = lut.tolist()


class Info:
    pass


def _be16(d, i):
    return d[i] << 8 | d[i + 1]


def parse(data) -> Info:
    """everything the host learns before the device is touched; raises Unsupported or Corrupt"""
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise _at(Corrupt("no SOI"), 0)
    s = Info()
    s.q, s.dc, s.ac = [None] * 4, [None] * 4, [None] * 4
    s.restart = 0
    frame, adobe = None, None
    pos = 2
    while True:
        if pos + 1 >= n or d[pos] != 0xFF:
            raise _at(Corrupt("marker expected"), pos)
        while pos + 1 < n and d[pos + 1] == 0xFF:
            pos += 1                                       # fill bytes
        if pos + 1 >= n:
            raise _at(Corrupt("file ends in a marker"), pos)
        m = d[pos + 1]
        pos += 2
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0xD8, 0xD9):
            raise _at(Corrupt("SOI / EOI before the scan"), pos - 2)
        if pos + 2 > n:
            raise _at(Corrupt("segment length"), pos)
        ln = _be16(d, pos)
        if ln < 2 or pos + ln > n:
            raise _at(Corrupt("segment length"), pos)
        body = d[pos + 2:pos + ln]
        if m in (0xC0, 0xC1):
            if frame is not None or len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise _at(Corrupt("SOF"), pos)
            if body[0] != 8:
                raise _at(Unsupported(f"{body[0]}-bit samples"), pos)
            s.h, s.w, s.nc = _be16(body, 1), _be16(body, 3), body[5]
            if s.h == 0:
                raise _at(Unsupported("height 0: DNL"), pos)
            if s.w == 0:
                raise _at(Corrupt("width 0"), pos)
            if s.nc not in (1, 3):
                raise _at(Unsupported(f"{s.nc} components"), pos)
            frame = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(s.nc)]
        elif m in (0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF):
            raise _at(Unsupported("progressive, lossless or arithmetic"), pos)
        elif m == 0xC4:
            i = 0
            while i < len(body):
                if i + 17 > len(body) or (body[i] >> 4) > 1 or (body[i] & 15) > 3:
                    raise _at(Corrupt("DHT"), pos)
                bits = body[i + 1:i + 17]
                cnt = sum(bits)
                if cnt > 256 or i + 17 + cnt > len(body):
                    raise _at(Corrupt("DHT"), pos)
                vals = body[i + 17:i + 17 + cnt]
                if (body[i] >> 4) == 0 and any(v > 15 for v in vals):
                    raise _at(Corrupt("DHT: DC category above 15"), pos)
                try:
                    (s.ac if body[i] >> 4 else s.dc)[body[i] & 15] = Huff(bits, vals)
                except Corrupt as e:
                    raise _at(e, pos)
                i += 17 + cnt
        elif m == 0xDB:
            i = 0
            while i < len(body):
                pq, tq = body[i] >> 4, body[i] & 15
                if pq > 1 or tq > 3 or i + 1 + 64 * (pq + 1) > len(body):
                    raise _at(Corrupt("DQT"), pos)
                t = np.zeros(64, np.int64)
                for k in range(64):
                    t[ZIGZAG[k]] = _be16(body, i + 1 + 2 * k) if pq else body[i + 1 + k]
                s.q[tq] = t
                i += 1 + 64 * (pq + 1)
        elif m == 0xDD:
            if ln != 4:
                raise _at(Corrupt("DRI"), pos)
            s.restart = _be16(body, 0)
        elif m == 0xDC:
            raise _at(Unsupported("DNL"), pos)
        elif m == 0xEE and len(body) >= 12 and body[:5] == b"Adobe":
            adobe = body[11]
        elif m == 0xDA:
            if frame is None or len(body) < 1 or len(body) != 4 + 2 * body[0]:
                raise _at(Corrupt("SOS"), pos)
            if body[0] != s.nc:
                raise _at(Unsupported("several scans"), pos)
            s.td, s.ta, s.tq = [], [], []
            for i in range(s.nc):
                if body[1 + 2 * i] != frame[i][0]:
                    raise _at(Unsupported("scan components out of order"), pos)
                td, ta = body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15
                if td > 3 or ta > 3 or s.dc[td] is None or s.ac[ta] is None or frame[i][3] > 3 or s.q[frame[i][3]] is None:
                    raise _at(Corrupt("a table the scan names is missing"), pos)
                s.td.append(td), s.ta.append(ta), s.tq.append(frame[i][3])
            if body[-3] != 0 or body[-2] != 63 or body[-1] != 0:
                raise _at(Unsupported("spectral selection or successive approximation"), pos)
            pos += ln
            break
        pos += ln
    if s.nc == 3 and adobe == 0:
        raise _at(Unsupported("Adobe transform 0: RGB"), pos)
    if s.nc == 1:
        s.hs = s.vs = 1                                     # (one component: not interleaved, whatever its factors)
    else:
        if (frame[1][1], frame[1][2], frame[2][1], frame[2][2]) != (1, 1, 1, 1) or (frame[0][1], frame[0][2]) not in ((1, 1), (2, 1), (2, 2)):
            raise _at(Unsupported("sampling factors"), pos)
        s.hs, s.vs = frame[0][1], frame[0][2]
    s.ny = s.hs * s.vs
    s.bpm = s.ny + (2 if s.nc == 3 else 0)
    s.comp = [0] * s.ny + ([1, 2] if s.nc == 3 else [])   # component of each block of an MCU
    s.mcux, s.mcuy = -(-s.w // (8 * s.hs)), -(-s.h // (8 * s.vs))
    s.nmcu = s.mcux * s.mcuy
    s.nblocks = s.nmcu * s.bpm
    s.interval = s.restart if s.restart else s.nmcu        # MCUs of a full segment
    s.nseg = -(-s.nmcu // s.interval)
    s.ibl = s.interval * s.bpm
    # the walk over the scan's 0xFF bytes: stuffed zeros, fill bytes and RSTm are removed; anything else ends the scan
    s.scan_start = pos
    removed, cuts, i = 0, [], pos
    while True:
        j = d.find(b"\xff", i)
        if j < 0 or j + 1 >= n:
            raise _at(Corrupt("no EOI"), n)
        nx = d[j + 1]
        if nx == 0:
            removed, i = removed + 1, j + 2
        elif nx == 0xFF:
            removed, i = removed + 1, j + 1
        elif 0xD0 <= nx <= 0xD7:
            if s.restart == 0 or nx - 0xD0 != len(cuts) & 7 or len(cuts) + 1 >= s.nseg:
                raise _at(Corrupt(f"RST{nx - 0xD0} at byte {j}"), j)
            cuts.append(j - pos - removed)
            removed, i = removed + 2, j + 2
        else:
            break
    if nx == 0xDC:
        raise _at(Unsupported("DNL"), j)
    if nx != 0xD9:
        raise _at(Unsupported("several scans"), j)
    if len(cuts) + 1 != s.nseg:
        raise _at(Corrupt("restart markers missing"), j)
    s.scan_len = j - pos
    s.segoff = [0] + cuts + [s.scan_len - removed]          # bytes of the unstuffed stream
    if any(b <= a for a, b in zip(s.segoff, s.segoff[1:])):
        raise _at(Corrupt("an empty segment"), pos)
    if s.scan_len >= (1 << 32) - 32:
        raise _at(Unsupported("a stuffed scan of 2 ** 32 bytes"), pos)
    if s.segoff[-1] * 8 >= 1 << 31:
        raise _at(Unsupported("a scan of 2 ** 31 bits"), pos)
    s.data = d
    return s


def unstuffed(s) -> bytes:
    """the segments back to back: 0x00 behind 0xFF, 0xFF fill bytes and RSTm dropped"""
    a = np.frombuffer(s.data, np.uint8, s.scan_len + 1, s.scan_start)
    cur, nxt, prev = a[:-1], a[1:], np.concatenate([[0], a[:-2]])
    drop = ((cur == 0xFF) & (nxt != 0)) | ((prev == 0xFF) & ((cur == 0) | ((cur >= 0xD0) & (cur <= 0xD7))))
    return cur[~drop].tobytes()


# ---- subsequences and the step function ------------------------------------------------------------------------------------------------
class Stream:
    def __init__(self, s, S=0):
        S = S or DEFAULT_SUBSEQ_BITS
        assert S % 32 == 0 and S >= 256
        self.s, self.S = s, S
        u = unstuffed(s)
        assert len(u) == s.segoff[-1]
        self.U = u + bytes(16)
        self.dc_lut = [s.dc[s.td[c]].lut for c in s.comp]
        self.ac_lut = [s.ac[s.ta[c]].lut for c in s.comp]
        self.subs = []                                      # (segment, first bit, end bit, the segment's end bit)
        self.subfirst = [0]
        for k in range(s.nseg):
            a, e = 8 * s.segoff[k], 8 * s.segoff[k + 1]
            self.subs += [(k, b, min(b + S, e), e) for b in range(a, e, S)]
            self.subfirst.append(len(self.subs))
        self.first = [i in set(self.subfirst) for i in range(len(self.subs))]

    def quota(self, k):
        """the blocks [first, end) the geometry gives segment k"""
        return k * self.s.ibl, min((k + 1) * self.s.ibl, self.s.nblocks)


def span(st, p, z, c, end, E, coef=None, b=0, bq=0):
    """The symbols that start in [p, end), from state (p, z, c).  Without ``coef``: F_i -- returns (exit state, blocks completed).  With
    it: the last pass -- writes block b onwards while b < bq and returns the bit of the first error, or None."""
    U, bpm, n = st.U, st.s.bpm, 0
    while p < end and (coef is None or b < bq):
        w = (int.from_bytes(U[p >> 3:(p >> 3) + 5], "big") >> (8 - (p & 7))) & 0xFFFFFFFF
        e = (st.dc_lut[c] if z == 0 else st.ac_lut[c])[w >> 16]
        if e == 0:                                          # no code: one bit
            if coef is not None:
                return p
            p += 1
            continue
        ln, sym = e >> 8, e & 255
        sz, run = (sym, 0) if z == 0 else (sym & 15, sym >> 4)
        if p + ln + sz > E:                                 # runs off the segment: stops at its end
            if coef is not None:
                return p
            p = E
            break
        v = (w >> (32 - ln - sz)) & ((1 << sz) - 1)
        if sz and v < 1 << (sz - 1):
            v -= (1 << sz) - 1
        p0, p = p, p + ln + sz
        if z == 0:
            if coef is not None:
                coef[b, 0] = v
            z = 1
            continue
        if sz == 0 and run != 15:                           # EOB
            z = 64
        else:
            z += run if sz else 16
            if z > 63:                                      # a run past index 63 ends the block
                if coef is not None:
                    return p0
            elif sz:
                if coef is not None:
                    coef[b, z] = v
                z += 1
            else:
                continue
        if z > 63:
            z, c, n, b = 0, (c + 1) % bpm, n + 1, b + 1
    return None if coef is not None else ((p, z, c), n)


def synchronise(st):
    """the fixed-point iteration: (entry states, blocks completed per subsequence, rounds)"""
    N = len(st.subs)
    entry = [(a, 0, 0) for _, a, _, _ in st.subs]
    memo = [None] * N
    rounds = 0
    while True:
        rounds += 1
        new = list(entry)
        for i, (k, a, e, E) in enumerate(st.subs):
            if memo[i] is None or memo[i][0] != entry[i]:   # (a state that did not change gives what it gave)
                memo[i] = (entry[i],) + span(st, *entry[i], e, E)
            if i + 1 < N and not st.first[i + 1]:
                new[i + 1] = memo[i][1]
        same, entry = new == entry, new
        if same:
            break
    assert rounds <= N + 1
    return entry, [m[2] for m in memo], rounds


def sequential(st, grid=True):
    """A plain decoder, written apart from ``span``: every segment from its start to its quota of blocks.  Returns (coefficients with
    the DC a difference, the state at the first symbol at or behind every subsequence's first bit)."""
    s = st.s
    coef = np.zeros((s.nblocks, 64), np.int16)
    states = [None] * len(st.subs)
    U = st.U

    def bits(p, n):
        return (int.from_bytes(U[p >> 3:(p >> 3) + 5], "big") >> (40 - (p & 7) - n)) & ((1 << n) - 1) if n else 0

    def symbol(h, p):
        code, k = 0, 0
        first = 0
        for n in range(1, 17):
            code = code << 1 | bits(p + n - 1, 1)
            if code - first < h.bits[n - 1]:
                return n, h.vals[k + code - first]
            k += h.bits[n - 1]
            first = (first + h.bits[n - 1]) << 1
        raise Corrupt(f"no code at bit {p}")

    def extend(v, n):
        return v - (1 << n) + 1 if n and v < 1 << (n - 1) else v

    for k in range(s.nseg):
        b, bq = st.quota(k)
        p, E = 8 * s.segoff[k], 8 * s.segoff[k + 1]
        marks = list(range(st.subfirst[k], st.subfirst[k + 1]))

        def note(p, z, c):
            while marks and st.subs[marks[0]][1] <= p:
                states[marks.pop(0)] = (p, z, c)

        while b < bq:
            c = (b % s.bpm)
            cc = s.comp[c]
            note(p, 0, c)
            n, sz = symbol(s.dc[s.td[cc]], p)
            if p + n + sz > E:
                raise Corrupt(f"segment {k} ends inside a symbol")
            coef[b, 0] = extend(bits(p + n, sz), sz)
            p += n + sz
            z = 1
            while z < 64:
                note(p, z, c)
                n, sym = symbol(s.ac[s.ta[cc]], p)
                run, sz = sym >> 4, sym & 15
                if p + n + sz > E:
                    raise Corrupt(f"segment {k} ends inside a symbol")
                if sz == 0 and run != 15:
                    p += n
                    break
                z += run if sz else 16
                if z > 63:
                    raise Corrupt(f"index past 63 at bit {p}")
                if sz:
                    coef[b, z] = extend(bits(p + n, sz), sz)
                    z += 1
                p += n + sz
            b += 1
        # what is left of the segment belongs to no block: the states there are whatever the iteration finds
    return coef, states


def coefficients(st, entry, counts):
    """the last pass: every subsequence from its true entry state into zeroed coefficients; raises Corrupt"""
    s = st.s
    coef = np.zeros((s.nblocks, 64), np.int16)
    first = np.concatenate([[0], np.cumsum(counts)])
    err = None
    for k in range(s.nseg):
        b0, bq = st.quota(k)
        i0, i1 = st.subfirst[k], st.subfirst[k + 1]
        if first[i1] - first[i0] != bq - b0:
            err = min(err, 8 * s.segoff[k]) if err is not None else 8 * s.segoff[k]
        for i in range(i0, i1):
            _, a, e, E = st.subs[i]
            r = span(st, *entry[i], e, E, coef, b0 + int(first[i] - first[i0]), bq)
            if r is not None:
                err = min(err, r) if err is not None else r
    if err is not None:
        raise Corrupt(f"bit {err} of the unstuffed scan")
    return coef


def dc_values(s, coef):
    """coefficients with the DC a value: an inclusive scan over the blocks ordered by component, minus its value where the block's
    segment begins"""
    out = coef.copy()
    b = np.arange(s.nblocks)
    mcu, k = b // s.bpm, b % s.bpm
    lum = k < s.ny
    pos = np.where(lum, mcu * s.ny + k, s.nmcu * s.ny + (k - s.ny) * s.nmcu + mcu)
    m0 = mcu // s.interval * s.interval
    pos0 = np.where(lum, m0 * s.ny, s.nmcu * s.ny + (k - s.ny) * s.nmcu + m0)
    d = np.zeros(s.nblocks, np.int64)
    d[pos] = coef[:, 0]
    ex = np.concatenate([[0], np.cumsum(d)])
    out[:, 0] = (ex[pos + 1] - ex[pos0]).astype(np.int16)  # (the low 16 bits, signed: INTEGRATION.md section 8 item 7; only a damaged stream wraps)
    return out


# ---- pixels --------------------------------------------------------------------------------------------------------------------------
def _idct_pass(d, shift):
    """one pass of libjpeg's accurate integer inverse DCT along the last axis (jidctint.c: 13-bit constants)"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    z1 = (d2 + d6) * 4433
    t2, t3 = z1 - d6 * 15137, z1 + d2 * 6270
    t0, t1 = (d0 + d4) << 13, (d0 - d4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d7, d5, d3, d1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    r = 1 << (shift - 1)
    return np.stack([(t10 + t3 + r) >> shift, (t11 + t2 + r) >> shift, (t12 + t1 + r) >> shift, (t13 + t0 + r) >> shift,
                     (t13 - t0 + r) >> shift, (t12 - t1 + r) >> shift, (t11 - t2 + r) >> shift, (t10 - t3 + r) >> shift], axis=-1)


def samples(s, coef):
    """(nblocks, 8, 8) uint8: dequantised, inverse transformed (columns, then rows), level shifted and clamped"""
    q = np.stack([s.q[s.tq[c]] for c in s.comp])           # (bpm, 64) row-major
    f = np.zeros((s.nblocks, 64), np.int64)
    f[:, ZIGZAG] = coef.astype(np.int64)
    f = np.clip(f * np.tile(q, (s.nmcu, 1)), -32768, 32767).reshape(-1, 8, 8)  # (saturated to 16 bits: the contract's range)
    cols = _idct_pass(f.transpose(0, 2, 1), 11).transpose(0, 2, 1)
    return np.clip(_idct_pass(cols, 18) + 128, 0, 255).astype(np.uint8)


def planes(s, coef):
    """the component planes, padded to whole MCUs"""
    blk = samples(s, coef).reshape(s.mcuy, s.mcux, s.bpm, 8, 8)
    y = blk[:, :, :s.ny].reshape(s.mcuy, s.mcux, s.vs, s.hs, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(s.mcuy * s.vs * 8, s.mcux * s.hs * 8)
    rest = [blk[:, :, s.ny + i].transpose(0, 2, 1, 3).reshape(s.mcuy * 8, s.mcux * 8) for i in range(s.nc - 1)]
    return [y] + rest


def _upsample(s, p):
    """one chroma plane at the frame's size: libjpeg's triangle filter where the plane is more than two samples wide, else replication"""
    h, w = s.h, s.w
    cw, ch = -(-w // s.hs), -(-h // s.vs)
    p = p[:ch, :cw].astype(np.int64)
    if s.hs == 1:
        return p
    x = np.arange(w)
    if cw <= 2:
        rows = p[np.arange(h) // s.vs] if s.vs == 2 else p
        return rows[:, x // 2]
    near = x // 2
    far = np.clip(near + np.where(x & 1, 1, -1), 0, cw - 1)
    if s.vs == 1:
        return (3 * p[:, near] + p[:, far] + np.where(x & 1, 2, 1)) >> 2
    y = np.arange(h)
    rn = y // 2
    rf = np.clip(rn + np.where(y & 1, 1, -1), 0, ch - 1)
    col = 3 * p[rn] + p[rf]                                # (h, cw) column sums
    return (3 * col[:, near] + col[:, far] + np.where(x & 1, 7, 8)) >> 4


def pixels(s, coef_dc, channels=3):
    """(h, w, 3) BGR, or (h, w) for a grey file and channels=1"""
    ps = planes(s, coef_dc)
    y = ps[0][:s.h, :s.w].astype(np.int64)
    if s.nc == 1:
        g = y.astype(np.uint8)
        return g if channels == 1 else np.stack([g, g, g], axis=-1)
    cb, cr = _upsample(s, ps[1]) - 128, _upsample(s, ps[2]) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


class Decoded:
    pass


def decode(data, S=0, channels=3, check=True) -> Decoded:
    """the whole contract for one file"""
    s = parse(data)
    st = Stream(s, S)
    r = Decoded()
    r.info, r.stream = s, st
    r.entry, r.counts, r.rounds = synchronise(st)
    r.segments, r.subsequences = s.nseg, len(st.subs)
    r.coef = coefficients(st, r.entry, r.counts)
    if check:
        coef, states = sequential(st)
        assert np.array_equal(coef, r.coef)
        assert all(a is None or a == b for a, b in zip(states, r.entry))
    r.pixels = pixels(s, dc_values(s, r.coef), channels)
    return r
