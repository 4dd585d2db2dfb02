"""NumPy / plain Python restatement of the device decoder of PROGRESSIVE JPEG files ("Progressive files"): the
contract in code.  What a progressive file shares with a sequential one -- the Huffman tables, unstuffing, the pixel stage -- is
imported from ``jpgdec_ref``; here is what is new: the parse over all the scans, the map from a scan's blocks to the MCU-major store,
the step functions of the four scan kinds, the iteration over the entry states, a plain decoder written apart from it, the last pass.

1. One zeroed int16 store ``coef[nblocks, 64]`` for the file, zigzag, MCU-major (what ``jpgdec_ref.pixels`` reads).  A scan of one
   component walks the component's OWN ceil(wc / 8) x ceil(hc / 8) blocks in raster order; ``block_of`` maps that to the store.
2. Scans run in file order; a scan's coefficients are final before the next scan's bits are read.
3. Inside a scan: segments from RSTm, subsequences of S bits, rounds until no entry state changes.  The state is (p, z, c, run, b):
   bit, zigzag index within the band, block within the scan's MCU, and -- in an AC refinement scan only, 0 elsewhere -- the blocks of
   an end-of-band run still to end and the block the state is in (the bits a block takes there depend on which of its coefficients are
   nonzero, so the block belongs to the state).  One step is one Huffman symbol with its extra and correction bits, or one block's
   share of a running end-of-band run; a DC refinement step is one bit; an EOBn symbol of an AC first scan ends its 2^n + extra
   blocks in one step.  Wrong entry states follow jpgdec_ref's rules: bits that start no code consume one bit, a run past the band's
   end ends the block, a step that would pass the segment's end stops the decode there, a refinement size above 1 counts as 1.
4. The last pass per scan writes the store and alone judges the stream; the earliest bad scan's smallest bad bit is reported.
5. Behind the last scan: ``jpgdec_ref.pixels``.
"""
from __future__ import annotations

import numpy as np

from jpgdec_ref import DEFAULT_SUBSEQ_BITS, Corrupt, Huff, Info, Unsupported, _at, _be16, pixels, unstuffed
from jpg_ref import ZIGZAG

DC_FIRST, DC_REFINE, AC_FIRST, AC_REFINE = 0, 1, 2, 3
COUNT_CAP = 0x40000000


# ---- the host-only parse ---------------------------------------------------------------------------------------------------------------
def parse(data) -> Info:
    """everything the host learns before the device is touched; raises Unsupported or Corrupt"""
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise _at(Corrupt("no SOI"), 0)
    s = Info()
    q, dc, ac = [None] * 4, [None] * 4, [None] * 4
    s.q, s.scans, s.data = [None] * 3, [], d
    restart, frame, adobe = 0, None, None
    bits = None
    pos = 2
    while True:
        if pos + 1 >= n or d[pos] != 0xFF:
            raise _at(Corrupt("marker expected"), pos)
        while pos + 1 < n and d[pos + 1] == 0xFF:
            pos += 1
        if pos + 1 >= n:
            raise _at(Corrupt("file ends in a marker"), pos)
        m = d[pos + 1]
        pos += 2
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            if not s.scans:
                raise _at(Corrupt("EOI before the scan"), pos - 2)
            break
        if m == 0xD8:
            raise _at(Corrupt("SOI"), pos - 2)
        if pos + 2 > n:
            raise _at(Corrupt("segment length"), pos)
        ln = _be16(d, pos)
        if ln < 2 or pos + ln > n:
            raise _at(Corrupt("segment length"), pos)
        body = d[pos + 2:pos + ln]
        if m == 0xC2:
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
            if s.nc == 1:
                s.hs = s.vs = 1
            else:
                if (frame[1][1], frame[1][2], frame[2][1], frame[2][2]) != (1, 1, 1, 1) or (frame[0][1], frame[0][2]) not in ((1, 1), (2, 1), (2, 2)):
                    raise _at(Unsupported("sampling factors"), pos)
                s.hs, s.vs = frame[0][1], frame[0][2]
            s.ny = s.hs * s.vs
            s.bpm = s.ny + (2 if s.nc == 3 else 0)
            s.comp = [0] * s.ny + ([1, 2] if s.nc == 3 else [])
            s.mcux, s.mcuy = -(-s.w // (8 * s.hs)), -(-s.h // (8 * s.vs))
            s.nmcu = s.mcux * s.mcuy
            s.nblocks = s.nmcu * s.bpm
            s.interval, s.nseg, s.ibl = s.nmcu, 1, s.nblocks     # (the pixel stage restarts nowhere)
            s.tq = list(range(s.nc))
            s.cw, s.ch = -(-s.w // s.hs), -(-s.h // s.vs)
            bits = [[-1] * 64 for _ in range(s.nc)]
        elif m in (0xC0, 0xC1):
            raise _at(Unsupported("a sequential file"), pos)
        elif m in (0xC3, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF):
            raise _at(Unsupported("lossless or arithmetic"), pos)
        elif m == 0xC4:
            i = 0
            while i < len(body):
                if i + 17 > len(body) or (body[i] >> 4) > 1 or (body[i] & 15) > 3:
                    raise _at(Corrupt("DHT"), pos)
                b16 = body[i + 1:i + 17]
                cnt = sum(b16)
                if cnt > 256 or i + 17 + cnt > len(body):
                    raise _at(Corrupt("DHT"), pos)
                vals = body[i + 17:i + 17 + cnt]
                if (body[i] >> 4) == 0 and any(v > 15 for v in vals):
                    raise _at(Corrupt("DHT: DC category above 15"), pos)
                try:
                    (ac if body[i] >> 4 else dc)[body[i] & 15] = Huff(b16, vals)
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
                q[tq] = t
                i += 1 + 64 * (pq + 1)
        elif m == 0xDD:
            if ln != 4:
                raise _at(Corrupt("DRI"), pos)
            restart = _be16(body, 0)
        elif m == 0xDC:
            raise _at(Unsupported("DNL"), pos)
        elif m == 0xEE and len(body) >= 12 and body[:5] == b"Adobe":
            adobe = body[11]
        elif m == 0xDA:
            if frame is None or len(body) < 1 or len(body) != 4 + 2 * body[0] or not 1 <= body[0] <= s.nc:
                raise _at(Corrupt("SOS"), pos)
            sc = Info()
            ns = body[0]
            Ss, Se, Ah, Al = body[-3], body[-2], body[-1] >> 4, body[-1] & 15
            if Ss > 63 or Se > 63 or Se < Ss or (Ss == 0 and Se != 0) or (Ss > 0 and ns != 1) or Al > 13:
                raise _at(Corrupt("an illegal scan"), pos)
            if Ah != 0 and Ah != Al + 1:
                raise _at(Corrupt("an illegal scan: a refinement by other than one bit"), pos)
            sc.kind = (AC_FIRST if Ss else DC_FIRST) + (1 if Ah else 0)
            sc.Ss, sc.Se, sc.Al, sc.Ah, sc.ni = Ss, Se, Al, Ah, ns == 1
            sc.comps, sc.jk, sc.jdc, sc.jc = [], [], [], []   # per block j of the scan's MCU: place in the file's MCU, DC table, component
            before = -1
            for i in range(ns):
                c = [k for k in range(s.nc) if frame[k][0] == body[1 + 2 * i]]
                if not c:
                    raise _at(Corrupt("SOS: no such component"), pos)
                c = c[-1]
                if c <= before:
                    raise _at(Unsupported("scan components out of order"), pos)
                before = c
                td, ta = body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15
                if td > 3 or ta > 3 or (sc.kind == DC_FIRST and dc[td] is None) or (sc.kind >= AC_FIRST and ac[ta] is None):
                    raise _at(Corrupt("a table the scan names is missing"), pos)
                if s.q[c] is None:
                    if frame[c][3] > 3 or q[frame[c][3]] is None:
                        raise _at(Corrupt("a table the scan names is missing"), pos)
                    s.q[c] = q[frame[c][3]].copy()
                for k in range(Ss, Se + 1):
                    if Ah == 0 and bits[c][k] != -1:
                        raise _at(Unsupported("a coefficient's first scan comes twice"), pos)
                    if Ah != 0 and bits[c][k] == -1:
                        raise _at(Corrupt("a refinement of a coefficient whose first scan never came"), pos)
                    if Ah != 0 and bits[c][k] != Ah:
                        raise _at(Corrupt("a refinement out of step"), pos)
                    bits[c][k] = Al
                sc.comps.append(c)
                sc.ac = ac[ta]
                for jc in range(1 if (c or ns == 1) else s.ny):
                    sc.jk.append(s.ny + c - 1 if c else jc), sc.jdc.append(dc[td]), sc.jc.append(c)
            if ns == 1:
                c = sc.comps[0]
                wc, hc = (s.cw, s.ch) if c else (s.w, s.h)
                sc.comp0, sc.bw = c, -(-wc // 8)
                sc.bps, sc.nmcu = 1, sc.bw * -(-hc // 8)
            else:
                sc.bps, sc.nmcu = len(sc.jk), s.nmcu
            sc.nunits = sc.nmcu * sc.bps
            sc.restart = restart
            interval = restart if restart else sc.nmcu
            sc.nseg, sc.ibl = -(-sc.nmcu // interval), interval * sc.bps
            pos += ln
            sc.scan_start, sc.data = pos, d
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
                    if restart == 0 or nx - 0xD0 != len(cuts) & 7 or len(cuts) + 1 >= sc.nseg:
                        raise _at(Corrupt(f"RST{nx - 0xD0} at byte {j}"), j)
                    cuts.append(j - pos - removed)
                    removed, i = removed + 2, j + 2
                else:
                    break
            if nx == 0xDC:
                raise _at(Unsupported("DNL"), j)
            if len(cuts) + 1 != sc.nseg:
                raise _at(Corrupt("restart markers missing"), j)
            sc.scan_len = j - pos
            sc.segoff = [0] + cuts + [sc.scan_len - removed]
            if sc.scan_len >= (1 << 32) - 32:
                raise _at(Unsupported("a stuffed scan of 2 ** 32 bytes"), pos)
            if sc.segoff[-1] * 8 >= 1 << 31:
                raise _at(Unsupported("a scan of 2 ** 31 bits"), pos)
            if any(b <= a for a, b in zip(sc.segoff, sc.segoff[1:])):
                raise _at(Corrupt("an empty segment"), pos)
            s.scans.append(sc)
            pos = j
            continue
        pos += ln
    if s.nc == 3 and adobe == 0:
        raise _at(Unsupported("Adobe transform 0: RGB"), pos)
    if any(b != 0 for row in bits for b in row):
        raise _at(Unsupported("the scans leave coefficients unfinished"), pos)
    return s


def block_of(s, sc, u):
    """the block of the file's MCU-major store that unit u of the scan is"""
    if sc.ni:
        by, bx = divmod(u, sc.bw)
        if sc.comp0 == 0:
            return ((by // s.vs) * s.mcux + bx // s.hs) * s.bpm + (by % s.vs) * s.hs + bx % s.hs
        return (by * s.mcux + bx) * s.bpm + s.ny + sc.comp0 - 1
    mcu, j = divmod(u, sc.bps)
    return mcu * s.bpm + sc.jk[j]


# ---- subsequences and the step function ------------------------------------------------------------------------------------------------
class Stream:
    def __init__(self, s, sc, S=0):
        S = S or DEFAULT_SUBSEQ_BITS
        assert S % 32 == 0 and S >= 256
        self.s, self.sc, self.S = s, sc, S
        u = unstuffed(sc)
        assert len(u) == sc.segoff[-1]
        self.U = u + bytes(16)
        self.subs, self.subfirst = [], [0]
        for k in range(sc.nseg):
            a, e = 8 * sc.segoff[k], 8 * sc.segoff[k + 1]
            self.subs += [(k, b, min(b + S, e), e) for b in range(a, e, S)]
            self.subfirst.append(len(self.subs))
        firsts = set(self.subfirst)
        self.first = [i in firsts for i in range(len(self.subs))]
        self.z0 = sc.Ss if sc.kind >= AC_FIRST else 0

    def quota(self, k):
        return k * self.sc.ibl, min((k + 1) * self.sc.ibl, self.sc.nunits)

    def seg_entry(self, k):
        return (8 * self.sc.segoff[k], self.z0, 0, 0, k * self.sc.ibl if self.sc.kind == AC_REFINE else 0)


def _w32(U, p):
    return (int.from_bytes(U[p >> 3:(p >> 3) + 5], "big") >> (8 - (p & 7))) & 0xFFFFFFFF


def _bit(U, p):
    return (U[p >> 3] >> (7 - (p & 7))) & 1


def _extend(v, n):
    return v - (1 << n) + 1 if n and v < 1 << (n - 1) else v


def _correct(blk, ks, U, q, Al):
    p1 = 1 << Al
    for k in ks:
        if _bit(U, q):
            c = int(blk[k])
            if c & p1 == 0:
                blk[k] = np.int16(c + p1 if c >= 0 else c - p1)
        q += 1


def span(st, coef, state, end, E, write=False, b=0, bq=0, dd=None):
    """The steps that start in [p, end) from ``state``; ``coef`` is the store (read by AC refinement scans, written when ``write``).
    Not ``write``: F_i -- returns (exit state, blocks completed).  ``write``: the last pass from unit b on while b < bq -- returns the
    bit of the first bad step, or None."""
    s, sc, U = st.s, st.sc, st.U
    p, z, c, run, sb = state
    if not write:
        b = sb
    n = 0
    Ss, Se, Al = sc.Ss, sc.Se, sc.Al
    err = None
    if sc.kind == DC_FIRST:
        while p < end and (not write or b < bq):
            w = _w32(U, p)
            e = sc.jdc[c].lut[w >> 16]
            if e == 0:
                if write:
                    err = p
                    break
                p += 1
                continue
            ln, sz = e >> 8, e & 15
            if p + ln + sz > E:
                if write:
                    err = p
                p = E
                break
            if write:
                dd[b] = _extend((w >> (32 - ln - sz)) & ((1 << sz) - 1), sz)
            p += ln + sz
            c = (c + 1) % sc.bps
            n, b = n + 1, b + 1
    elif sc.kind == DC_REFINE:
        if not write:
            if p < end:
                n, p = end - p, end
        else:
            while p < end and b < bq:
                if _bit(U, p):
                    coef[block_of(s, sc, b), 0] |= np.int16(1 << Al)
                p, n, b = p + 1, n + 1, b + 1
    elif sc.kind == AC_FIRST:
        lut = sc.ac.lut
        while p < end and (not write or b < bq):
            w = _w32(U, p)
            e = lut[w >> 16]
            if e == 0:
                if write:
                    err = p
                    break
                p += 1
                continue
            ln, sym = e >> 8, e & 255
            sz, rn = sym & 15, sym >> 4
            extra = sz if sz else (rn if rn < 15 else 0)
            if p + ln + extra > E:
                if write:
                    err = p
                p = E
                break
            raw = (w >> (32 - ln - extra)) & ((1 << extra) - 1)
            p0, p = p, p + ln + extra
            done, blocks = False, 1
            if sz == 0 and rn < 15:
                blocks = (1 << rn) + raw
                if write and blocks > bq - b:
                    err = p0
                    break
                done = True
            else:
                z += rn if sz else 16
                if z > Se:
                    if write:
                        err = p0
                        break
                    done = True
                elif sz:
                    if write:
                        coef[block_of(s, sc, b), z] = np.array(_extend(raw, sz) << Al).astype(np.int16)
                    z += 1
                    done = z > Se
            if done:
                z, n, b = Ss, min(n + blocks, COUNT_CAP), b + blocks
    else:
        lut = sc.ac.lut
        while (p < end or (end == E and run > 0)) and (not write or b < bq):
            blk = coef[block_of(s, sc, b)] if b < sc.nunits else None
            nzs = [k for k in range(Ss, Se + 1) if blk is not None and blk[k] != 0]
            if run > 0:
                ks = [k for k in nzs if k >= z]
                if p + len(ks) > E:
                    if write:
                        err = p
                    p = E
                    break
                if write:
                    _correct(blk, ks, U, p, Al)
                p, run, z, n, b = p + len(ks), run - 1, Ss, n + 1, (b + 1) & 0xFFFFFFFF
                continue
            w = _w32(U, p)
            e = lut[w >> 16]
            if e == 0:
                if write:
                    err = p
                    break
                p += 1
                continue
            ln, sym = e >> 8, e & 255
            sz, rn = sym & 15, sym >> 4
            if sz == 0 and rn < 15:
                if p + ln + rn > E:
                    if write:
                        err = p
                    p = E
                    break
                run = (1 << rn) + ((w >> (32 - ln - rn)) & ((1 << rn) - 1))
                p += ln + rn
                continue
            if write and sz > 1:
                err = p
                break
            need = ln + (1 if sz else 0)
            zeros = [k for k in range(z, Se + 1) if k not in nzs]
            kz = zeros[rn] if rn < len(zeros) else Se + 1
            ks = [k for k in nzs if z <= k < kz]
            if p + need + len(ks) > E:
                if write:
                    err = p
                p = E
                break
            if write:
                if kz > Se:
                    err = p
                    break
                _correct(blk, ks, U, p + need, Al)
                if sz:
                    blk[kz] = np.int16((1 << Al) if _bit(U, p + ln) else -(1 << Al))
            p += need + len(ks)
            z = kz + 1
            if z > Se:
                z, n, b = Ss, n + 1, (b + 1) & 0xFFFFFFFF
    if write:
        return err
    return (p, z, c, run, b if sc.kind == AC_REFINE else 0), n


def synchronise(st, coef):
    """the fixed-point iteration of one scan: (entry states, blocks completed per subsequence, rounds)"""
    N = len(st.subs)
    entry = [st.seg_entry(k) if st.first[i] else (a, st.z0, 0, 0, 0) for i, (k, a, _, _) in enumerate(st.subs)]
    memo = [None] * N
    rounds = 0
    while True:
        rounds += 1
        new = list(entry)
        for i, (k, a, e, E) in enumerate(st.subs):
            if memo[i] is None or memo[i][0] != entry[i]:
                memo[i] = (entry[i],) + span(st, coef, entry[i], e, E)
            if i + 1 < N and not st.first[i + 1]:
                new[i + 1] = memo[i][1]
        same, entry = new == entry, new
        if same:
            break
    assert rounds <= N + 1
    return entry, [m[2] for m in memo], rounds


def last_pass(st, coef, entry, counts):
    """every subsequence from its true entry state into the store; raises Corrupt with the smallest bad bit"""
    s, sc = st.s, st.sc
    first = np.concatenate([[0], np.cumsum(counts)])
    dd = [0] * sc.nunits
    err = None
    for k in range(sc.nseg):
        b0, bq = st.quota(k)
        i0, i1 = st.subfirst[k], st.subfirst[k + 1]
        total = int(first[i1] - first[i0])
        if total < bq - b0 if sc.kind == DC_REFINE else total != bq - b0:
            err = min(err, 8 * sc.segoff[k]) if err is not None else 8 * sc.segoff[k]
        for i in range(i0, i1):
            _, a, e, E = st.subs[i]
            r = span(st, coef, entry[i], e, E, True, min(b0 + int(first[i] - first[i0]), bq), bq, dd)
            if r is not None:
                err = min(err, r) if err is not None else r
    if err is not None:
        raise Corrupt(f"bit {err} of the unstuffed scan")
    if sc.kind == DC_FIRST:                                  # the prediction per component, restarted at every segment
        pred = {}
        for u in range(sc.nunits):
            if u % sc.ibl == 0:
                pred = {}
            c = sc.jc[u % sc.bps]
            pred[c] = pred.get(c, 0) + dd[u]
            coef[block_of(s, sc, u), 0] = np.array(pred[c] << sc.Al).astype(np.int16)


def plain_scan(st, coef):
    """A plain decoder of one scan after libjpeg's jdphuff.c, written apart from ``span``: every segment from its start to its quota
    of blocks, into ``coef``.  Returns the state at the first step at or behind every subsequence's first bit (None where the
    segment's blocks end before it)."""
    s, sc, U = st.s, st.sc, st.U
    states = [None] * len(st.subs)
    Ss, Se, Al = sc.Ss, sc.Se, sc.Al
    p1 = 1 << Al

    def symbol(h, p):
        code, k, first = 0, 0, 0
        for n in range(1, 17):
            code = code << 1 | _bit(U, p + n - 1)
            if code - first < h.bits[n - 1]:
                return n, h.vals[k + code - first]
            k += h.bits[n - 1]
            first = (first + h.bits[n - 1]) << 1
        raise Corrupt(f"no code at bit {p}")

    def take(p, n):
        v = 0
        for i in range(n):
            v = v << 1 | _bit(U, p + i)
        return v

    for k in range(sc.nseg):
        b, bq = st.quota(k)
        p, E = 8 * sc.segoff[k], 8 * sc.segoff[k + 1]
        marks = list(range(st.subfirst[k], st.subfirst[k + 1]))
        refine = sc.kind == AC_REFINE

        def note(p, z, c, run=0):
            while marks and st.subs[marks[0]][1] <= p:
                states[marks.pop(0)] = (p, z, c, run, b if refine else 0)

        pred, eobrun = {}, 0
        while b < bq:
            j = (b - k * sc.ibl) % sc.bps
            blk = coef[block_of(s, sc, b)]
            if sc.kind == DC_FIRST:
                note(p, 0, j)
                n, sz = symbol(sc.jdc[j], p)
                if p + n + sz > E:
                    raise Corrupt("segment ends inside a symbol")
                c = sc.jc[j]
                pred[c] = pred.get(c, 0) + _extend(take(p + n, sz), sz)
                blk[0] = np.array(pred[c] << Al).astype(np.int16)
                p += n + sz
            elif sc.kind == DC_REFINE:
                note(p, 0, 0)
                if p + 1 > E:
                    raise Corrupt("segment ends inside a symbol")
                if _bit(U, p):
                    blk[0] |= np.int16(p1)
                p += 1
            elif sc.kind == AC_FIRST:
                if eobrun:
                    eobrun -= 1
                else:
                    z = Ss
                    while z <= Se:
                        note(p, z, 0)
                        n, sym = symbol(sc.ac, p)
                        r, sz = sym >> 4, sym & 15
                        if sz:
                            z += r
                            if z > Se or p + n + sz > E:
                                raise Corrupt(f"bad symbol at bit {p}")
                            blk[z] = np.array(_extend(take(p + n, sz), sz) << Al).astype(np.int16)
                            p += n + sz
                            z += 1
                        elif r == 15:
                            if z + 16 > Se or p + n > E:
                                raise Corrupt(f"bad symbol at bit {p}")
                            z, p = z + 16, p + n
                        else:
                            if p + n + r > E:
                                raise Corrupt(f"bad symbol at bit {p}")
                            eobrun = (1 << r) + take(p + n, r) - 1
                            p += n + r
                            if eobrun > bq - b - 1:
                                raise Corrupt(f"an end-of-band run past the segment at bit {p}")
                            break
            else:
                z = Ss
                if eobrun == 0:
                    while z <= Se:
                        note(p, z, 0)
                        n, sym = symbol(sc.ac, p)
                        r, sz = sym >> 4, sym & 15
                        if sz == 0 and r < 15:
                            if p + n + r > E:
                                raise Corrupt(f"bad symbol at bit {p}")
                            eobrun = (1 << r) + take(p + n, r)
                            p += n + r
                            break
                        if sz > 1:
                            raise Corrupt(f"bad symbol at bit {p}")
                        new = 0
                        q = p + n
                        if sz:
                            new = p1 if _bit(U, q) else -p1
                            q += 1
                        while z <= Se:                          # libjpeg's inner loop over the coefficients the symbol passes
                            if blk[z] != 0:
                                if q >= E:
                                    raise Corrupt(f"bad symbol at bit {p}")
                                if _bit(U, q) and int(blk[z]) & p1 == 0:
                                    blk[z] += np.int16(p1 if blk[z] >= 0 else -p1)
                                q += 1
                            else:
                                r -= 1
                                if r < 0:
                                    break
                            z += 1
                        if z > Se or q > E:
                            raise Corrupt(f"bad symbol at bit {p}")
                        if new:
                            blk[z] = np.int16(new)
                        z, p = z + 1, q
                if eobrun > 0:
                    note(p, z, 0, eobrun)
                    while z <= Se:
                        if blk[z] != 0:
                            if p >= E:
                                raise Corrupt(f"segment ends inside a run at bit {p}")
                            if _bit(U, p) and int(blk[z]) & p1 == 0:
                                blk[z] += np.int16(p1 if blk[z] >= 0 else -p1)
                            p += 1
                        z += 1
                    eobrun -= 1
            b += 1
        if eobrun:
            raise Corrupt("an end-of-band run past the segment")
    return states


class Decoded:
    pass


def decode(data, S=0, channels=3, check=True, keep_scans=False) -> Decoded:
    """the whole contract for one file"""
    s = parse(data)
    r = Decoded()
    r.info = s
    coef = np.zeros((s.nblocks, 64), np.int16)
    r.scan_rounds, r.entries, r.counts, r.after = [], [], [], []
    r.segments = r.subsequences = 0
    for n, sc in enumerate(s.scans):
        st = Stream(s, sc, S)
        before = coef.copy() if check else None
        entry, counts, rounds = synchronise(st, coef)
        try:
            last_pass(st, coef, entry, counts)
        except Corrupt as e:
            raise Corrupt(f"scan {n}: {e}") from e
        if check:
            states = plain_scan(st, before)
            assert np.array_equal(before, coef), f"scan {n}: the iteration and the plain decoder disagree"
            assert all(a is None or a == b for a, b in zip(states, entry)), f"scan {n}: states"
        r.scan_rounds.append(rounds), r.entries.append(entry), r.counts.append(counts)
        if keep_scans:
            r.after.append(coef.copy())
        r.segments, r.subsequences = r.segments + sc.nseg, r.subsequences + len(st.subs)
    r.scans, r.rounds = len(s.scans), sum(r.scan_rounds)
    r.coef = coef
    r.pixels = pixels(s, coef, channels)
    return r
