"""The progressive JPEG files the device decoder is tested on (tests/test_jpegprog_host.py, tests/test_gpu_jpegprog.py).

Two generators.  (a) Pillow with ``progressive=True``: libjpeg-turbo's default script of ten scans with successive approximation (six
for a grey image).  (b) ``progressive`` below, a small writer after libjpeg's jcphuff.c that takes quantised coefficients and ANY legal
script, with Huffman tables of each scan's own histogram (``jpg_opt_ref.optimal_table``, coded by ``jpg_ref.code_table``) in a DHT in
front of every scan: it reaches what Pillow cannot write.  Every file must decode in Pillow (``pillow_pixels``), so the writer is not
its own judge.
"""
from __future__ import annotations

import functools
import io
import struct

import numpy as np

import jpg_cases as PC
import jpg_opt_ref as OR
import jpg_ref as R
import jpgdec_cases as DC
import jpgdec_ref as D
import jpgprog_ref as P

SUBSEQ = (256, 1024)


def pillow_pixels(data, grey=False):
    """Pillow's decode as cv2 orders it: (h, w, 3) BGR, or (h, w) of a grey file with ``grey``"""
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    if im.mode == "L":
        a = np.asarray(im)
        return a if grey else np.stack([a, a, a], axis=-1)
    return np.asarray(im.convert("RGB"))[..., ::-1]


# ---- the writer -----------------------------------------------------------------------------------------------------------------------
def scan(comps, Ss, Se, Ah, Al, dri=None):
    """one entry of a script; ``dri``: a DRI segment of this value in front of the scan (0 switches restarts off)"""
    return dict(comps=list(comps), Ss=Ss, Se=Se, Ah=Ah, Al=Al, dri=dri)


def _units(g, comps):
    """(block of the MCU-major store, component) of every block of a scan, in the scan's order, and the blocks of one of its MCUs"""
    ny, bpm = g.hs * g.vs, g.hs * g.vs + (2 if g.nc == 3 else 0)
    mcux, mcuy = -(-g.w // (8 * g.hs)), -(-g.h // (8 * g.vs))
    out = []
    if len(comps) == 1:
        c = comps[0]
        wc, hc = (g.w, g.h) if c == 0 else (-(-g.w // g.hs), -(-g.h // g.vs))
        for by in range(-(-hc // 8)):
            for bx in range(-(-wc // 8)):
                if c == 0:
                    out.append((((by // g.vs) * mcux + bx // g.hs) * bpm + (by % g.vs) * g.hs + bx % g.hs, c))
                else:
                    out.append(((by * mcux + bx) * bpm + ny + c - 1, c))
        return out, 1
    per = [(k, 0) for k in range(ny)] if 0 in comps else []
    per += [(ny + c - 1, c) for c in comps if c]
    for m in range(mcux * mcuy):
        out += [(m * bpm + k, c) for k, c in per]
    return out, len(per)


def _size(v):
    return int(abs(int(v))).bit_length()


class _Tokens:
    """a segment's symbols and raw bits, in order"""

    def __init__(self):
        self.t = []

    def sym(self, s):
        self.t.append(("s", s))

    def bits(self, v, n):
        if n:
            self.t.append(("b", v & ((1 << n) - 1), n))


def _scan_tokens(zz, units, bps, sc, interval):
    """the scan as one _Tokens per segment (jcphuff.c: encode_mcu_DC_first, _AC_first, _DC_refine, _AC_refine, emit_eobrun)"""
    Ss, Se, Ah, Al = sc["Ss"], sc["Se"], sc["Ah"], sc["Al"]
    segs = []
    per = interval * bps if interval else len(units)
    for a in range(0, len(units), per):
        T = _Tokens()
        pred, eobrun, be = {}, 0, []

        def flush():
            nonlocal eobrun, be
            if eobrun:
                n = eobrun.bit_length() - 1
                T.sym(n << 4)
                T.bits(eobrun, n)
                eobrun = 0
            for b in be:
                T.bits(b, 1)
            be = []

        for blk, c in units[a:a + per]:
            v = zz[blk]
            if Ss == 0 and Ah == 0:
                t = int(v[0]) >> Al
                d = t - pred.get(c, 0)
                pred[c] = t
                n = _size(d)
                T.sym(n)
                T.bits(d if d >= 0 else d - 1, n)
            elif Ss == 0:
                T.bits(int(v[0]) >> Al, 1)
            elif Ah == 0:
                r = 0
                for k in range(Ss, Se + 1):
                    t = int(v[k])
                    m = abs(t) >> Al
                    if m == 0:
                        r += 1
                        continue
                    flush()
                    while r > 15:
                        T.sym(0xF0)
                        r -= 16
                    n = m.bit_length()
                    T.sym(r << 4 | n)
                    T.bits(m if t >= 0 else ~m, n)
                    r = 0
                if r > 0:
                    eobrun += 1
                    if eobrun == 0x7FFF:
                        flush()
            else:
                ab = [abs(int(v[k])) >> Al for k in range(64)]
                eob = max([k for k in range(Ss, Se + 1) if ab[k] == 1], default=0)
                r, br = 0, []
                for k in range(Ss, Se + 1):
                    t = ab[k]
                    if t == 0:
                        r += 1
                        continue
                    while r > 15 and k <= eob:
                        flush()
                        T.sym(0xF0)
                        r -= 16
                        for b in br:
                            T.bits(b, 1)
                        br = []
                    if t > 1:
                        br.append(t & 1)
                        continue
                    flush()
                    T.sym(r << 4 | 1)
                    T.bits(0 if v[k] < 0 else 1, 1)
                    for b in br:
                        T.bits(b, 1)
                    br, r = [], 0
                if r > 0 or br:
                    eobrun += 1
                    be += br
                    if eobrun == 0x7FFF or len(be) > 937:
                        flush()
        flush()
        segs.append(T.t)
    return segs


def _entropy_bytes(tokens, code, length):
    acc, n, out = 0, 0, bytearray()
    for t in tokens:
        if t[0] == "s":
            v, k = int(code[t[1]]), int(length[t[1]])
            assert k
        else:
            v, k = t[1], t[2]
        acc, n = acc << k | v, n + k
        while n >= 8:
            n -= 8
            b = (acc >> n) & 255
            out.append(b)
            if b == 0xFF:
                out.append(0)
        acc &= (1 << n) - 1
    if n:
        b = (acc << (8 - n) | ((1 << (8 - n)) - 1)) & 255
        out.append(b)
        if b == 0xFF:
            out.append(0)
    return bytes(out)


def progressive(zz, g, qts, script, table=None) -> bytes:
    """A progressive file of the quantised coefficients ``zz`` ((nblocks, 64), zigzag, MCU-major, DC as values), geometry ``g`` (h, w,
    nc, hs, vs), quantisation tables ``qts`` (row-major, luma and chroma) and the scans of ``script``.  ``table(counts, ac, k)``: the
    (table spec, slot 0 ... 3) of scan ``k`` from its symbol counts; None: the optimal table in slot 0."""
    out = bytearray(b"\xff\xd8")
    out += DC.segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate(qts[:1 if g.nc == 1 else 2]):
        out += DC.segment(0xDB, bytes([i]) + bytes(int(q[R.ZIGZAG[k]]) for k in range(64)))
    sof = struct.pack(">BHHB", 8, g.h, g.w, g.nc)
    for c in range(g.nc):
        sof += bytes([c + 1, (g.hs << 4 | g.vs) if c == 0 and g.nc == 3 else 0x11, 0 if c == 0 else 1])
    out += DC.segment(0xC2, sof)
    interval = 0
    for k, sc in enumerate(script):
        if sc["dri"] is not None:
            interval = sc["dri"]
            out += DC.segment(0xDD, struct.pack(">H", interval))
        units, bps = _units(g, sc["comps"])
        segs = _scan_tokens(zz, units, bps, sc, interval)
        counts = np.zeros(256, np.int64)
        for seg in segs:
            for t in seg:
                if t[0] == "s":
                    counts[t[1]] += 1
        code = length = None
        slot = 0
        if counts.any():
            spec, slot = (OR.optimal_table(counts), 0) if table is None else table(counts, bool(sc["Ss"]), k)
            code, length = R.code_table(spec)
            out += DC.segment(0xC4, bytes([(0x10 if sc["Ss"] else 0x00) | slot]) + bytes(spec[0]) + bytes(spec[1]))
        out += DC.segment(0xDA, bytes([len(sc["comps"])]) + b"".join(bytes([c + 1, slot << 4 | slot]) for c in sc["comps"]) +
                          bytes([sc["Ss"], sc["Se"], sc["Ah"] << 4 | sc["Al"]]))
        for i, seg in enumerate(segs):
            if i:
                out += bytes([0xFF, 0xD0 + (i - 1) % 8])
            out += _entropy_bytes(seg, code, length)
    return bytes(out + b"\xff\xd9")


class _G:
    def __init__(self, h, w, nc, hs=1, vs=1):
        self.h, self.w, self.nc, self.hs, self.vs = h, w, nc, hs, vs
        self.nblocks = -(-w // (8 * hs)) * -(-h // (8 * vs)) * (hs * vs + (2 if nc == 3 else 0))


def from_sequential(data, script) -> bytes:
    """the coefficients of a sequential file, written again by ``script``"""
    r = D.decode(data, check=False)
    s = r.info
    return progressive(D.dc_values(s, r.coef), _G(s.h, s.w, s.nc, s.hs, s.vs), [s.q[s.tq[0]], s.q[s.tq[-1]]], script)


def full(comps, al=0):
    """DC interleaved, then every component's whole AC band, at point transform ``al`` with its refinements"""
    sc = [scan(comps, 0, 0, 0, al)] + [scan([c], 1, 63, 0, al) for c in comps]
    for a in range(al, 0, -1):
        sc += [scan(comps, 0, 0, a, a - 1)] + [scan([c], 1, 63, a, a - 1) for c in comps]
    return sc


# ---- the list -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def supported_cases() -> dict:
    c = {}
    pil = functools.partial(DC.pillow, progressive=True)
    # (a) Pillow: samplings x qualities, with and without restart markers; the sizes whose component grids are narrower than the MCUs'
    for i, s in enumerate(("gray", "444", "422", "420")):
        cn = 1 if s == "gray" else 3
        for j, q in enumerate((30, 90, 100)):
            h, w = ((17, 13), (33, 47), (24, 40))[j]
            c[f"pil_{s}_q{q}"] = pil(PC.smooth(h, w, cn, 100 + 4 * j + i), q, "420" if cn == 1 else s)
        c[f"pil_{s}_rst"] = pil(PC.smooth(33, 47, cn, 120 + i), 90, "420" if cn == 1 else s, restart_marker_blocks=2)
    c["pil_8x8_gray"] = pil(PC.smooth(8, 8, 1, 130), 90)
    c["pil_8x8_420"] = pil(PC.smooth(8, 8, 3, 131), 90, "420")
    c["pil_17x13_420"] = pil(PC.noise(17, 13, 3, 132), 90, "420")
    c["pil_17x13_422"] = pil(PC.noise(17, 13, 3, 133), 90, "422")
    c["pil_13x17_420"] = pil(PC.noise(13, 17, 3, 148), 90, "420")
    c["pil_13x17_422"] = pil(PC.noise(13, 17, 3, 149), 90, "422")
    c["pil_noise_q100_444"] = pil(PC.noise(64, 96, 3, 134), 100, "444")
    c["pil_noise_q100_gray"] = pil(PC.noise(64, 96, 1, 135), 100)
    flat = np.full((256, 256), 120, np.uint8)
    flat[128:136, 64:72] = PC.noise(8, 8, 1, 136).reshape(8, 8)
    c["pil_flat_one_block"] = pil(flat, 90)
    c["pil_128_dri1"] = pil(PC.smooth(128, 128, 1, 137), 75, restart_marker_blocks=1)
    c["pil_128_dri1_420"] = pil(PC.smooth(128, 128, 3, 138), 50, "420", restart_marker_blocks=1)
    # (b) the writer
    b420 = DC.pillow(PC.noise(33, 47, 3, 140) // 2 + PC.smooth(33, 47, 3, 141) // 2, 90, "420")
    b422 = DC.pillow(PC.noise(13, 17, 3, 142) // 2 + PC.smooth(13, 17, 3, 143) // 2, 90, "422")
    b444 = DC.pillow(PC.noise(24, 40, 3, 144) // 2 + PC.smooth(24, 40, 3, 145) // 2, 95, "444")
    bgray = DC.pillow(PC.noise(17, 13, 1, 146), 90)
    c["w_selection_only_420"] = from_sequential(b420, [scan([0, 1, 2], 0, 0, 0, 0)] +
                                                [scan([k], a, e, 0, 0) for k in (0, 1, 2) for a, e in ((1, 5), (6, 63))])
    c["w_dc_per_component_422"] = from_sequential(b422, [scan([k], 0, 0, 0, 0) for k in (2, 0, 1)] + [scan([k], 1, 63, 0, 0) for k in (1, 0, 2)])
    c["w_dc_two_components_420"] = from_sequential(b420, [scan([0], 0, 0, 0, 0), scan([1, 2], 0, 0, 0, 1), scan([1, 2], 0, 0, 1, 0)] +
                                                   [scan([k], 1, 63, 0, 0) for k in (0, 1, 2)])
    c["w_one_coefficient_bands"] = from_sequential(bgray, [scan([0], 0, 0, 0, 0)] + [scan([0], k, k, 0, 0) for k in range(1, 64)])
    c["w_al2_444"] = from_sequential(b444, full([0, 1, 2], 2))
    c["w_al2_420"] = from_sequential(b420, full([0, 1, 2], 2))
    c["w_al3_gray_dri"] = from_sequential(bgray, [dict(s, dri=1 + i % 3) for i, s in enumerate(full([0], 3))])
    s = full([0, 1, 2], 1)
    s[0]["dri"], s[1]["dri"], s[4]["dri"], s[6]["dri"] = 2, 5, 0, 1
    c["w_dri_changed_420"] = from_sequential(b420, s)
    # an end-of-band run of 32767 blocks (and one more block): a first scan ends it in one step
    g = _G(1024, 2048, 1)
    zz = np.zeros((g.nblocks, 64), np.int16)
    zz[:, 0] = 3
    zz[-1, 5] = -2
    q16 = np.full(64, 16, np.int64)
    c["w_eobrun_32767"] = progressive(zz, g, [q16, q16], full([0], 1))
    # a refinement scan that is one end-of-band run of correction bits over many subsequences: every coefficient nonzero at Al = 1
    # already, none new at Al = 0
    g = _G(64, 64, 1)
    rng = np.random.default_rng(147)
    zz = (rng.integers(1, 4, (g.nblocks, 64)) * 2 + rng.integers(0, 2, (g.nblocks, 64))).astype(np.int16) * rng.choice([-1, 1], (g.nblocks, 64))
    zz[:, 20:] = 0
    c["w_correction_run"] = progressive(zz.astype(np.int16), g, [q16, q16], full([0], 1))
    return c


@functools.lru_cache(maxsize=None)
def unsupported_cases() -> dict:
    """files the host parse hands to the host reader"""
    b420 = DC.pillow(PC.smooth(33, 47, 3, 150), 90, "420")
    s = full([0, 1, 2], 1)
    return {
        "incomplete_no_refinement": from_sequential(b420, s[:4]),                # every coefficient stops at bit 1
        "incomplete_band": from_sequential(b420, [scan([0, 1, 2], 0, 0, 0, 0)] + [scan([k], 1, 20, 0, 0) for k in (0, 1, 2)]),
        "incomplete_component": from_sequential(b420, [scan([0, 1, 2], 0, 0, 0, 0), scan([0], 1, 63, 0, 0), scan([1], 1, 63, 0, 0)]),
        "sequential": b420,
        "first_scan_twice": from_sequential(b420, [scan([0, 1, 2], 0, 0, 0, 0)] + full([0, 1, 2])),
    }


def _edit_sos(data, nth, **kw):
    """the file with fields of its nth SOS changed: Ss, Se, AhAl"""
    pos, k = 0, -1
    while True:
        pos = data.index(b"\xff\xda", pos + 1)
        k += 1
        if k == nth:
            break
    ln = struct.unpack(">H", data[pos + 2:pos + 4])[0]
    body = bytearray(data[pos + 4:pos + 2 + ln])
    for name, at in (("Ss", -3), ("Se", -2), ("AhAl", -1)):
        if name in kw:
            body[at] = kw[name]
    return data[:pos + 4] + bytes(body) + data[pos + 2 + ln:]


@functools.lru_cache(maxsize=None)
def corrupt_cases() -> dict:
    """name: (file, whether the parse alone finds it)"""
    b420 = DC.pillow(PC.smooth(33, 47, 3, 151), 90, "420")
    ok = from_sequential(b420, full([0, 1, 2], 1))
    pil = supported_cases()["pil_noise_q100_444"]
    third = [i for i in range(len(pil) - 1) if pil[i] == 0xFF and pil[i + 1] == 0xDA][2]
    nxt = pil.index(b"\xff\xc4", third)
    two = ok.replace(b"\xff\xda\x00\x08\x01\x01\x00", b"\xff\xda\x00\x0a\x02\x01\x00\x02\x00", 1)
    return {
        "ac_scan_of_two_components": (two, True),
        "dc_scan_with_band": (_edit_sos(ok, 0, Se=5), True),
        "refinement_by_two_bits": (_edit_sos(ok, 4, AhAl=0x20), True),
        "refinement_without_first": (from_sequential(b420, [scan([0, 1, 2], 0, 0, 1, 0)] + full([0, 1, 2])), True),
        "refinement_out_of_step": (_edit_sos(from_sequential(b420, full([0, 1, 2], 2)), 4, AhAl=0x10), True),
        "no_eoi": (ok[:-2], True),
        "truncated_third_scan": (pil[:nxt - 3] + pil[nxt:], False),
    }


TRUNCATED = "truncated_third_scan"  # the corrupt case that also runs on the device


@functools.lru_cache(maxsize=None)
def reference(name, S=0):
    """the restatement of a supported case"""
    return P.decode(supported_cases()[name], S, check=False, keep_scans=True)
