"""Legal JPEG files that no encoder here writes, and files with one damaged header, for the device decoders and the lossless entries:
shared by the host half (tests/test_jpegodd_host.py, and the stand-alone sanitizer runs it starts), the GPU half
(tests/test_gpu_jpegodd.py) and the fuzz slice (tools/fuzz.py --jpegodd).  Nothing is committed: the lists are built on first use and
cached, the same bytes on every machine.

``legal()``: LEGAL_SEQ sequential and LEGAL_PROG progressive files.  The coefficients are those of small Pillow files (1 x 1 to 48 x 48;
grey, 4:4:4, 4:2:2, 4:2:0; smooth, noise and flat; qualities 30 / 90 / 100) as the restatement reads them; ``write`` codes them again
with what a ``Plan`` says: Huffman tables of drawn shape (``code_lengths``) in drawn slots, quantisation tables in drawn slots with 8- or
16-bit entries, decoy definitions, arbitrary component ids, a grey frame with sampling factors, fill bytes, segment orders, COM / APPn
sizes and DRI oddities.  A file's ``tags`` name what it holds; tests/test_jpegodd_host.py asserts that every tag of TAGS occurs in at
least two files of different sampling, and that the group ``complete`` -- tables whose Kraft sum is 1, so that the all-ones word of
the longest length is a code: libjpeg refuses them, the product decodes them -- is exactly a quarter.
The progressive files get the same code shapes and slots per scan through ``jpgprog_cases.progressive(table=...)``.

``header_damage(prog)``: DAMAGE_SEQ sequential and DAMAGE_PROG progressive files, each a small supported case with one damage drawn
from DAMAGE_SEED in the bytes that tests/jpgdmg_cases.py leaves alone: the marker segments.  Kinds (KINDS): ``length`` (a length field +-1,
+-2, 0, 1 or 65535), ``field`` (Nf, Ns, Hi/Vi, Tq, Td/Ta, Tc/Th, Pq, one of the sixteen BITS, Ss/Se/Ah/Al, the DRI value), ``dimension``
(0 or 65535), ``drop``, ``duplicate``, ``exchange`` (two neighbouring segments), ``cut_boundary`` and ``cut_inside``.  ``verdict`` is
the restatement's: ``parsed`` (with what jpgdmg_cases.verdict_of says of the file), ``unsupported`` or ``corrupt``, with the byte the
parse refuses the file at.  By the restatement, as tests/test_jpegodd_host.py prints and asserts (parsed / unsupported / corrupt):

    sequential, 96 files: 24 / 12 / 60 (of the 24 parsed files 16 decode and 8 are refused by the last pass)
        length 0/0/10   field 3/5/18   dimension 6/3/3   drop 1/0/9   duplicate 6/4/0   exchange 8/0/2   cut_boundary 0/0/9
        cut_inside 0/0/9
    progressive, 48 files: 9 / 8 / 31 (of the 9 parsed files 6 decode and 3 are refused by the last pass)
        length 0/0/7    field 3/5/14   dimension 1/2/2   drop 0/1/2   duplicate 3/0/1   exchange 2/0/1   cut_boundary 0/0/2
        cut_inside 0/0/2

The variants of ``length``, ``field`` and ``dimension`` are taken in rotation (VARIANTS), so that each list holds every length edit, every
dimension and every named field -- the sixteen BITS and the DRI value, which decide lookup contents and launch sizes, among them --
and ``Damaged.sub`` names a file's; one BITS damage per list moves a code to the next length (the table parses, with another shape);
Td / Ta come again with slots above 3, the first one past the tables among them.
"""
from __future__ import annotations

import functools
import struct
from collections import namedtuple

import numpy as np

import jpg_cases as PC
import jpg_ref as R
import jpgdec_cases as DC
import jpgdec_ref as D
import jpgdmg_cases as M
import jpgprog_cases as PCS
import jpgprog_ref as P

SEED = 7
DAMAGE_SEED = {False: 37, True: 42}   # per list; picked so that each holds enough files of every verdict (tests/test_jpegodd_host.py asserts it)
SUBSEQ = (256, 1024)
LUT_BITS = 8                    # kLutBits of jpegdec_core.hpp: longer codes take the maxcode / valoff path
LEGAL_SEQ, LEGAL_PROG = 48, 16
DAMAGE_SEQ, DAMAGE_PROG = 96, 48
SAMPLINGS = ("gray", "444", "422", "420")
SIZES = ((1, 1), (7, 9), (16, 16), (17, 33), (40, 48), (48, 48), (24, 40), (33, 17))
QUALITIES = (30, 90, 100)

# what a legal file can hold; every one in at least two files of different sampling
TAGS = ("random", "long", "one1", "one16", "unused_dc", "unused_ac", "complete", "slots", "decoy_same_segment", "decoy_two_segments",
        "unnamed_table", "tq_slots", "dqt8", "dqt16", "dqt16_high", "dqt_redefined", "ids", "fill", "fill_rst", "fill_eoi", "dri_first", "dht_first",
        "dqt_last", "com2", "app65535", "two_dri", "dri_large")
GREY_TAGS = ("grey_2x2", "grey_1x2")   # (a grey frame's own: "different sampling" is the two of them)

Case = namedtuple("Case", "name data sampling group tags prog")


def _rng(*key):
    return np.random.default_rng([SEED, *key])


# ---- code shapes ----------------------------------------------------------------------------------------------------------------------
def code_lengths(n, rng, shape) -> list:
    """the code lengths (1 ... 16) of ``n`` symbols, Kraft-feasible: ``random`` (a drawn binary tree with one leaf left free, some codes
    made longer still), ``complete`` (the tree with no leaf free: the Kraft sum is 1), ``long`` (every length above LUT_BITS),
    ``one1`` / ``one16`` (n = 1: a code of 1 bit, of 16 bits)"""
    if shape == "one1" or shape == "one16":
        assert n == 1
        return [1 if shape == "one1" else 16]
    if shape == "long":
        out = [int(v) for v in rng.integers(LUT_BITS + 1, 17, n)]
    else:
        assert n >= (2 if shape == "complete" else 1)
        leaves = [0]
        while len(leaves) < n + (shape != "complete"):
            ok = [i for i, d in enumerate(leaves) if d < 16]
            deep = max(leaves[i] for i in ok)
            i = [j for j in ok if leaves[j] == deep][0] if rng.integers(2) else ok[int(rng.integers(len(ok)))]
            leaves[i] += 1
            leaves.append(leaves[i])
        if shape != "complete":
            leaves.remove(max(leaves))
            for i in range(n):
                if rng.integers(4) == 0:
                    leaves[i] = int(rng.integers(leaves[i], 17))
        out = leaves
    k = sum(1 << (16 - v) for v in out)
    assert len(out) == n and min(out) >= 1 and max(out) <= 16 and (k == 1 << 16 if shape == "complete" else k < 1 << 16)
    return out


def table_spec(symbols, rng, shape):
    """(BITS, HUFFVAL) of the symbols, HUFFVAL in drawn order"""
    syms = [int(v) for v in rng.permutation(sorted(symbols))]
    ln = sorted(code_lengths(len(syms), rng, shape))
    return [ln.count(i) for i in range(1, 17)], syms


def kraft(spec):
    """the Kraft sum of a table spec times 2 ** 16"""
    return sum(b << (16 - i) for i, b in enumerate(spec[0], 1))


UNUSED_DC = (12, 13, 14, 15)
UNUSED_AC = (0x0B, 0x1C, 0x2D, 0x3E, 0xFF, 0x0F, 0xFB)


def _shaped(used, rng, shape, ac):
    """the table spec of one table of a file of ``shape`` and the tags it earns"""
    used = set(used)
    tags = set()
    if shape in ("one1", "one16"):
        if len(used) == 1:
            return table_spec(used, rng, shape), {shape}
        shape = "random"
    if shape in ("unused", "complete"):
        extra = [v for v in (UNUSED_AC if ac else UNUSED_DC) if rng.integers(2) or shape == "unused"] or [15]
        if shape == "unused" or len(used) < 2:
            used |= set(extra)
            tags.add("unused_ac" if ac else "unused_dc")
        if shape == "unused":
            shape = "random"
    else:
        used |= {int(v) for v in rng.integers(0, 16 if not ac else 256, int(rng.integers(3)))}  # (a few further symbols, used or not)
    tags.add(shape)
    return table_spec(used, rng, shape), tags


# ---- the writer -----------------------------------------------------------------------------------------------------------------------
class Plan:
    """what ``write`` makes of a file's coefficients.  Per component: ``ids``, ``td``, ``ta``, ``tq`` (slots), ``factors`` (the SOF's
    sampling byte).  ``dht``: the DHT segments, each a list of (Tc << 4 | Th, spec), in order -- a later definition of a slot rules.
    ``dqt``: the DQT segments, each a list of (Pq, Tq, 64 row-major entries).  ``restart``: the interval in force (0: none);
    ``dri``: the values of the DRI segments, in order (the last is ``restart``).  ``order``: the segments' order, of "app0", "dqt",
    "sof", "dht", "dri", "extra".  ``fill``: 0xFF fill bytes in front of header markers / of RSTm / of EOI.  ``extra``: further
    segments (COM, APPn)."""
    order = ("app0", "dqt", "sof", "dht", "dri", "extra")
    fill = (False, False, False)
    extra = ()


def _codes(spec):
    code, length = R.code_table(spec)
    return [int(v) for v in code], [int(v) for v in length]


def entropy_segments(s, dcv, plan, specs_dc, specs_ac) -> list:
    """the stuffed bytes of every restart segment: ``dcv`` (nblocks, 64) zigzag, MCU-major, the DC a value; ``specs_*``: per component"""
    dc = [_codes(t) for t in specs_dc]
    ac = [_codes(t) for t in specs_ac]
    interval = plan.restart or s.nmcu
    out = []
    for m0 in range(0, s.nmcu, interval):
        acc, n, raw = 0, 0, bytearray()
        pred = [0] * s.nc

        def put(v, k):
            nonlocal acc, n
            acc, n = acc << k | v, n + k
            while n >= 8:
                n -= 8
                raw.append((acc >> n) & 255)
            acc &= (1 << n) - 1

        for b in range(m0 * s.bpm, min(m0 + interval, s.nmcu) * s.bpm):
            c = s.comp[b % s.bpm]
            v = dcv[b]
            d = int(v[0]) - pred[c]
            pred[c] = int(v[0])
            k = abs(d).bit_length()
            assert dc[c][1][k], (c, k)
            put(dc[c][0][k], dc[c][1][k])
            put((d if d >= 0 else d - 1) & ((1 << k) - 1), k)
            run = 0
            for z in range(1, 64):
                t = int(v[z])
                if t == 0:
                    run += 1
                    continue
                while run > 15:
                    put(ac[c][0][0xF0], ac[c][1][0xF0])
                    run -= 16
                k = abs(t).bit_length()
                assert ac[c][1][run << 4 | k]
                put(ac[c][0][run << 4 | k], ac[c][1][run << 4 | k])
                put((t if t >= 0 else t - 1) & ((1 << k) - 1), k)
                run = 0
            if run:
                assert ac[c][1][0]
                put(ac[c][0][0], ac[c][1][0])
        if n:
            put((1 << (8 - n)) - 1, 8 - n)
        out.append(bytes(raw).replace(b"\xff", b"\xff\x00"))
    return out


def used_symbols(s, dcv, restart):
    """per component: (the DC categories, the AC symbols) that coding the file with this interval emits"""
    interval = restart or s.nmcu
    dc, ac = [set() for _ in range(s.nc)], [set() for _ in range(s.nc)]
    pred = [0] * s.nc
    for b in range(s.nblocks):
        if b % (interval * s.bpm) == 0:
            pred = [0] * s.nc
        c = s.comp[b % s.bpm]
        v = dcv[b]
        dc[c].add(abs(int(v[0]) - pred[c]).bit_length())
        pred[c] = int(v[0])
        nz = np.nonzero(v[1:])[0] + 1
        last = 0
        for z in nz:
            run = int(z) - last - 1
            if run > 15:
                ac[c].add(0xF0)
            ac[c].add((run & 15) << 4 | abs(int(v[z])).bit_length())
            last = int(z)
        if last < 63:
            ac[c].add(0)
    return dc, ac


def write(s, dcv, plan) -> bytes:
    """the sequential file of coefficients ``dcv`` under geometry ``s`` (a jpgdec_ref parse) as ``plan`` says"""
    wide = any(pq for seg in plan.dqt for pq, _, _ in seg)
    seg = {"app0": [DC.segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")], "extra": list(plan.extra)}
    seg["dqt"] = [DC.segment(0xDB, b"".join(bytes([pq << 4 | tq]) + (b"".join(struct.pack(">H", int(t[k])) for k in R.ZIGZAG) if pq else
                                                                    bytes(int(t[k]) for k in R.ZIGZAG)) for pq, tq, t in g)) for g in plan.dqt]
    comps = b"".join(bytes([plan.ids[i], plan.factors[i], plan.tq[i]]) for i in range(s.nc))
    seg["sof"] = [DC.segment(0xC1 if wide else 0xC0, struct.pack(">BHHB", 8, s.h, s.w, s.nc) + comps)]
    seg["dht"] = [DC.segment(0xC4, b"".join(bytes([tc]) + bytes(sp[0]) + bytes(sp[1]) for tc, sp in g)) for g in plan.dht]
    seg["dri"] = [DC.segment(0xDD, struct.pack(">H", v)) for v in plan.dri]
    sos = DC.segment(0xDA, bytes([s.nc]) + b"".join(bytes([plan.ids[i], plan.td[i] << 4 | plan.ta[i]]) for i in range(s.nc)) + b"\x00\x3f\x00")
    head = [x for name in plan.order for x in seg[name]] + [sos]
    assert sorted(plan.order) == sorted(Plan.order)
    out = b"\xff\xd8" + b"".join((b"\xff" * (1 + k % 3) if plan.fill[0] else b"") + x for k, x in enumerate(head))
    # the tables in force: the last definition of every slot
    inforce = {tc: sp for g in plan.dht for tc, sp in g}
    segs = entropy_segments(s, dcv, plan, [inforce[plan.td[i]] for i in range(s.nc)], [inforce[0x10 | plan.ta[i]] for i in range(s.nc)])
    for k, x in enumerate(segs):
        if k:
            out += (b"\xff" * (1 + k % 2) if plan.fill[1] else b"") + bytes([0xFF, 0xD0 + (k - 1) % 8])
        out += x
    return out + (b"\xff\xff\xff" if plan.fill[2] else b"") + b"\xff\xd9"


# ---- the legal list -------------------------------------------------------------------------------------------------------------------
SHAPES = ("random", "long", "one1", "random", "unused", "one16", "long")


def _image(k, sampling, shape):
    h, w = SIZES[(k // 4 + k) % len(SIZES)]
    cn = 1 if sampling == "gray" else 3
    if shape in ("one1", "one16"):      # flat: every block is its DC and an end of block, and at 128 the DC is 0 too
        return np.full((h, w, cn)[:2 if cn == 1 else 3], 128 if k & 8 else 77, np.uint8)
    return (PC.noise if (k // 2) & 1 else PC.smooth)(h, w, cn, 300 + k)


def source(k, sampling, shape):
    """(the parse, the coefficients with the DC a value) of file k's Pillow file"""
    data = DC.pillow(_image(k, sampling, shape), QUALITIES[k % 3], "420" if sampling == "gray" else sampling)
    r = D.decode(data, check=False)
    return r.info, D.dc_values(r.info, r.coef)


def is_complete(k) -> bool:
    return (k // 4) % 4 == k % 4


def sequential_plan(k, s, dcv, rng, complete):
    """file k's Plan and tags"""
    p = Plan()
    tags = set()
    shape = "complete" if complete else SHAPES[k % 7]
    # restart: none, 1, 2, an MCU row, 3; a value above the MCU count; two DRI segments
    p.restart = (0, 1, 2, s.mcux, 3)[k % 5]
    if shape in ("one1", "one16") and s.nc == 3 and (s.hs, s.vs) == (1, 1):
        p.restart = 1                    # (every DC difference the same: one category per table)
    if k % 5 == 3 and not p.restart:
        p.restart = 2
    p.dri = [p.restart] if p.restart else []
    if k % 7 == 2 and shape not in ("one1", "one16"):
        p.restart = s.nmcu + 1 + int(rng.integers(60000))
        p.dri = [p.restart]
    if p.restart > s.nmcu:
        tags.add("dri_large")
    if k % 5 == 1 and p.restart:
        p.dri = [p.restart + 5] + p.dri
        tags.add("two_dri")
    # Huffman tables: every component its own pair of slots
    p.td = [int(v) for v in rng.permutation(4)[:s.nc]]
    p.ta = [int(v) for v in rng.permutation(4)[:s.nc]]
    tags.add("slots")
    used_dc, used_ac = used_symbols(s, dcv, p.restart)
    defs = []
    for c in range(s.nc):
        for ac in (0, 1):
            spec, t = _shaped((used_ac if ac else used_dc)[c], rng, shape, ac)
            tags |= t
            defs.append((ac << 4 | (p.ta if ac else p.td)[c], spec))
    decoy = lambda tc: (tc, _shaped({0, 1, 2}, rng, "random", tc >> 4)[0])
    if k % 3 == 2:                       # a table no component names
        free = [t for t in range(4) if t not in p.td]
        defs.insert(int(rng.integers(len(defs) + 1)), decoy(free[0]))
        tags.add("unnamed_table")
    if k % 6 == 1:                       # a slot defined twice within one segment, the decoy first
        p.dht = [[decoy(defs[1][0])] + defs]
        tags.add("decoy_same_segment")
    elif k % 6 == 4:                     # ... and across two segments
        p.dht = [[decoy(defs[0][0])], defs]
        tags.add("decoy_two_segments")
    elif k % 2:
        p.dht = [[d] for d in defs]
    else:
        p.dht = [defs]
    # quantisation tables: the file's two, in drawn slots; the chrominance components share a slot or name two with the same entries
    tq = [int(v) for v in rng.permutation(4)[:s.nc]]
    if s.nc == 3 and rng.integers(2):
        tq[2] = tq[1]
    p.tq = tq
    wide = k % 5 == 2
    qdefs = [(int(wide and (c != 1 or k % 2)), tq[c], s.q[s.tq[c]]) for c in range(s.nc) if c < 2 or tq[c] != tq[1]]
    if wide:
        # entries that need their high byte, in the luminance table: 65535 and 4660 where no block has a coefficient, and the largest
        # entry that keeps the product inside 2000 (libjpeg's sample range limit wraps far outside 0 ... 255: no yardstick there) at the position whose
        # largest coefficient is smallest -- so that the high byte decides pixels ("dqt16_high")
        peak = np.abs(dcv[[b for b in range(s.nblocks) if s.comp[b % s.bpm] == 0], 1:].astype(np.int64)).max(axis=0)
        big = s.q[s.tq[0]].copy()
        for z, v in zip([z + 1 for z in range(63) if peak[z] == 0][:2], (65535 - k % 200, 4660)):
            big[R.ZIGZAG[z]] = v
        live = [(int(v), z + 1) for z, v in enumerate(peak) if 0 < v <= 7]
        if live:
            v, z = min(live)
            big[R.ZIGZAG[z]] = 2000 // v
            tags.add("dqt16_high")
        qdefs[0] = (1, tq[0], big)
    tags |= {"tq_slots"} | {"dqt16" if pq else "dqt8" for pq, _, _ in qdefs}
    p.dqt = [qdefs] if k % 2 else [[d] for d in qdefs]
    if k % 7 == 3:
        p.dqt = [[(int(wide), qdefs[0][1], np.full(64, 1 + k % 200 + (300 if wide else 0)))]] + p.dqt
        tags.add("dqt_redefined")
    # the frame
    p.ids = [1, 2, 3][:s.nc]
    if k % 3 == 1:
        p.ids = [int(v) for v in rng.permutation(256)[:s.nc]]
        tags.add("ids")
    p.factors = [s.hs << 4 | s.vs, 0x11, 0x11][:s.nc]
    if s.nc == 1 and (k // 4) % 3:
        p.factors = [(0x22, 0x12)[(k // 4) % 3 - 1]]
        tags.add(("grey_2x2", "grey_1x2")[(k // 4) % 3 - 1])
    # layout
    if k % 5 == 3:
        p.fill = (True, True, True)
        tags |= {"fill", "fill_eoi"} | ({"fill_rst"} if s.nmcu > p.restart else set())
    order = (k // 3) % 4
    if order == 1:
        p.order = ("dri", "app0", "dqt", "sof", "dht", "extra")
        tags.add("dri_first")
    elif order == 2:
        p.order = ("app0", "dht", "extra", "dqt", "sof", "dri")
        tags.add("dht_first")
    elif order == 3:
        p.order = ("app0", "sof", "dri", "dht", "extra", "dqt")
        tags.add("dqt_last")
    if "dri_first" in tags and not p.dri:
        tags.discard("dri_first")
    if k % 7 == 5:
        p.extra = (DC.segment(0xFE, b""), DC.segment(0xE5, bytes(rng.integers(0, 256, 65533, dtype=np.uint8))))
        tags |= {"com2", "app65535"}
    return p, tags


def _prog_table(rng, shape, tags):
    def table(counts, ac, k):
        used = set(int(v) for v in np.nonzero(counts)[0])
        spec, t = _shaped(used, rng, shape, ac)
        tags.update(t | {"slots"})
        return spec, int(rng.integers(4))
    return table


@functools.lru_cache(maxsize=None)
def legal() -> tuple:
    out = []
    for k in range(LEGAL_SEQ):
        sampling = SAMPLINGS[k % 4]
        complete = is_complete(k)
        shape = "complete" if complete else SHAPES[k % 7]
        s, dcv = source(k, sampling, shape)
        plan, tags = sequential_plan(k, s, dcv, _rng(1, k), complete)
        out.append(Case(f"seq{k:02d}_{sampling}_{s.h}x{s.w}_{shape}", write(s, dcv, plan), sampling, "complete" if complete else "open",
                        frozenset(tags), False))
    for k in range(LEGAL_PROG):
        sampling = SAMPLINGS[k % 4]
        complete = is_complete(k)
        shape = "complete" if complete else ("random", "long", "unused")[k % 3]
        s, dcv = source(100 + k, sampling, shape)
        data, tags = progressive_file(k, s, dcv, _rng(2, k), shape)
        out.append(Case(f"prog{k:02d}_{sampling}_{s.h}x{s.w}_{shape}", data, sampling, "complete" if complete else "open", frozenset(tags), True))
    assert len(out) <= 64 and len({x.name for x in out}) == len(out)
    return tuple(out)


def legal_case(name) -> Case:
    return next(x for x in legal() if x.name == name)


@functools.lru_cache(maxsize=None)
def legal_reference(name, S):
    """the restatement's decode of a legal file"""
    x = legal_case(name)
    return (P if x.prog else D).decode(x.data, S, check=False)


def progressive_file(k, s, dcv, rng, shape):
    """progressive file k of coefficients ``dcv``: (the file, its tags)"""
    script = PCS.full(list(range(s.nc)), k % 3)
    if k % 5 == 2:
        script[0]["dri"] = 2
    tags = set()
    data = PCS.progressive(dcv, PCS._G(s.h, s.w, s.nc, s.hs, s.vs), [s.q[s.tq[0]], s.q[s.tq[-1]]], script, _prog_table(rng, shape, tags))
    return data, tags


def random_legal(rng):
    """one further file of the generator, one in four progressive, for the fuzz slice: (description, file, whether it is progressive)"""
    sampling = SAMPLINGS[int(rng.integers(4))]
    complete = bool(rng.integers(4) == 0)
    prog = bool(rng.integers(4) == 0)
    k = int(rng.integers(1 << 20))
    shape = "complete" if complete else ("random", "long", "unused")[k % 3] if prog else SHAPES[k % 7]
    s, dcv = source(k, sampling, shape)
    if prog:
        data, tags = progressive_file(k, s, dcv, rng, shape)
    else:
        plan, tags = sequential_plan(k, s, dcv, rng, complete)
        data = write(s, dcv, plan)
    return f"odd legal k={k} {sampling} {s.h}x{s.w} {shape} " + ",".join(sorted(tags)), data, prog


# ---- header damage --------------------------------------------------------------------------------------------------------------------
KINDS = ("length", "field", "dimension", "drop", "duplicate", "exchange", "cut_boundary", "cut_inside")
SEQ_BASES = ("size_8x8_gray", "size_8x8_444", "size_17x17_420", "size_15x33_422", "dri1_gray", "optimised_gray", "com_app1", "dqt16_sof1")
PROG_BASES = ("pil_gray_q30", "pil_444_q30", "pil_422_q30", "pil_420_q30", "pil_gray_rst", "w_al3_gray_dri")

# files of each kind
SEQ_PLAN = dict(length=10, field=26, dimension=12, drop=10, duplicate=10, exchange=10, cut_boundary=9, cut_inside=9)
PROG_PLAN = dict(length=7, field=22, dimension=5, drop=3, duplicate=4, exchange=3, cut_boundary=2, cut_inside=2)
# the variants of a kind, taken in rotation so that each list holds every one of them (a base without the field -- no DRI segment --
# passes it on to the next base that has it); Td / Ta come again: their values above 3 are what the parse's bound checks are for
LENGTHS = ("+1", "-1", "+2", "-2", "0", "1", "65535")
FIELDS = ("Nf", "Ns", "Hi", "Vi", "Tq", "Td", "Ta", "Tc", "Th", "Pq", "BITS", "Ss", "Se", "Ah", "Al", "DRI")
# ("BITS>": one code moved to the next length -- two neighbouring counts, their sum kept --, so that the segment still parses and the table
# has another shape: a single changed count moves every byte behind it and ends at the parse's length checks)
FIELD_ROTATION = FIELDS + ("Td", "Ta", "BITS>", "DRI", "Td", "Ta", "Tq", "Th", "Ns", "Nf")
DIMENSIONS = ("height 0", "height 65535", "width 0", "width 65535")
PROG_FIELD_ROTATION = FIELDS + ("Al", "Se", "Hi", "Vi", "Al", "BITS>")   # (what leaves a progressive file legal and outside the decoder's scope)
VARIANTS = {"length": LENGTHS, "field": FIELD_ROTATION, "dimension": DIMENSIONS}

Damaged = namedtuple("Damaged", "name data kind base prog sub how")   # sub: the variant (of LENGTHS, FIELDS, DIMENSIONS) or None
HVerdict = namedtuple("HVerdict", "what pos why inner")   # what: parsed / unsupported / corrupt; inner: jpgdmg_cases.Verdict of a parsed file


def segments(data) -> list:
    """[(marker, first byte of its 0xFF, byte behind the segment)] of every marker segment of a sound file, those between the scans of a
    progressive file included; the entropy-coded bytes and EOI are no segment"""
    out, pos, n = [], 2, len(data)
    while pos + 3 < n:
        assert data[pos] == 0xFF, pos
        while data[pos + 1] == 0xFF:                       # (fill bytes: the segment begins at the last of them)
            pos += 1
        m = data[pos + 1]
        if m == 0xD9:
            break
        end = pos + 2 + struct.unpack(">H", data[pos + 2:pos + 4])[0]
        out.append((m, pos, end))
        pos = end
        if m == 0xDA:
            while not (data[pos] == 0xFF and data[pos + 1] not in (0, 0xFF) and not 0xD0 <= data[pos + 1] <= 0xD7):
                pos += 1
    return out


def _fields(data, segs):
    """[(byte, mask, name)] of the counts and nibbles of the headers"""
    f = []
    for m, a, e in segs:
        b = a + 4
        if m in (0xC0, 0xC1, 0xC2):
            nf = data[b + 5]
            f.append((b + 5, 0xFF, "Nf"))
            for i in range(nf):
                f += [(b + 7 + 3 * i, 0xF0, "Hi"), (b + 7 + 3 * i, 0x0F, "Vi"), (b + 8 + 3 * i, 0xFF, "Tq")]
        elif m == 0xDA:
            ns = data[b]
            f.append((b, 0xFF, "Ns"))
            for i in range(ns):
                f += [(b + 2 + 2 * i, 0xF0, "Td"), (b + 2 + 2 * i, 0x0F, "Ta")]
            f += [(e - 3, 0xFF, "Ss"), (e - 2, 0xFF, "Se"), (e - 1, 0xF0, "Ah"), (e - 1, 0x0F, "Al")]
        elif m == 0xC4:
            i = b
            while i < e:
                f += [(i, 0xF0, "Tc"), (i, 0x0F, "Th")] + [(i + 1 + j, 0xFF, "BITS") for j in range(16)]
                i += 17 + sum(data[i + 1:i + 17])
        elif m == 0xDB:
            i = b
            while i < e:
                f += [(i, 0xF0, "Pq"), (i, 0x0F, "Tq")]
                i += 1 + 64 * ((data[i] >> 4) + 1)
        elif m == 0xDD:
            f += [(b, 0xFF, "DRI"), (b + 1, 0xFF, "DRI")]
    return f


def header_damage_of(data, kind, rng, sub=None):
    """(what was done, the variant, the file) with one damage of ``kind`` in the marker segments of the sound file ``data``; ``sub``: which
    variant of VARIANTS[kind] (None: drawn); KeyError where the file has no such field"""
    segs = segments(data)
    b = bytearray(data)
    k = int(rng.integers(len(segs)))
    m, a, e = segs[k]
    if kind == "length":
        ln = e - a - 2
        sub = sub or LENGTHS[int(rng.integers(7))]
        new = dict(zip(LENGTHS, (ln + 1, ln - 1, ln + 2, ln - 2, 0, 1, 65535)))[sub]
        if new == ln:                                      # (a segment of that length already: the neighbouring value)
            new -= 1
        b[a + 2:a + 4] = struct.pack(">H", new)
        return f"length of {m:02X} {ln} -> {new}", sub, bytes(b)
    if kind == "field":
        f = _fields(data, segs)
        names = sorted({x[2] for x in f})
        name = sub or names[int(rng.integers(len(names)))]    # (the field first: the sixteen BITS of every table would crowd the rest out)
        if name == "BITS>" or (sub is None and name == "BITS" and rng.integers(2)):
            pick = [x[0] for x, y in zip(f, f[1:]) if x[2] == y[2] == "BITS" and y[0] == x[0] + 1 and b[x[0]] and b[y[0]] < 255]
            at = pick[int(rng.integers(len(pick)))]
            b[at], b[at + 1] = b[at] - 1, b[at + 1] + 1
            return f"BITS at bytes {at}, {at + 1}: one code moved to the next length", "BITS", bytes(b)
        pick = [x for x in f if x[2] == name]
        if not pick:
            raise KeyError(name)
        at, mask, _ = pick[int(rng.integers(len(pick)))]
        old = b[at] & mask
        while (b[at] & mask) == old:
            if name in ("Td", "Ta") and rng.integers(3):      # a slot above 3: the first one past the tables half of the time
                v = 4 if rng.integers(2) else int(rng.integers(5, 16))
            else:
                v = int(rng.integers(0, 4)) if rng.integers(2) else int(rng.integers(0, 256))
            b[at] = (b[at] & ~mask & 255) | ((v << 4 if mask == 0xF0 else v) & mask)
        return f"{name} at byte {at}: {data[at]:02X} -> {b[at]:02X}", name, bytes(b)
    if kind == "dimension":
        m, a, e = next(x for x in segs if x[0] in (0xC0, 0xC1, 0xC2))
        sub = sub or DIMENSIONS[int(rng.integers(4))]
        which, v = int(sub.startswith("width")), int(sub.split()[1])
        b[a + 5 + 2 * which:a + 7 + 2 * which] = struct.pack(">H", v)
        return sub, sub, bytes(b)
    if kind == "drop":
        return f"{m:02X} dropped", None, data[:a] + data[e:]
    if kind == "duplicate":
        return f"{m:02X} twice", None, data[:e] + data[a:e] + data[e:]
    if kind == "exchange":
        k = int(rng.integers(len(segs) - 1))
        (m, a, e), (m2, a2, e2) = segs[k], segs[k + 1]
        if a2 != e:                                        # (a scan lies between them: the second goes in front of the first's header)
            return f"{m:02X} and {m2:02X} exchanged around a scan", None, data[:a] + data[a2:e2] + data[a:a2] + data[e2:]
        return f"{m:02X} and {m2:02X} exchanged", None, data[:a] + data[a2:e2] + data[a:e] + data[e2:]
    if kind == "cut_boundary":
        at = (a, e)[int(rng.integers(2))]
        return f"cut at byte {at}, a boundary of {m:02X}", None, data[:at]
    if kind == "cut_inside":
        at = (a + 1, a + 3, e - 1)[int(rng.integers(3))]
        return f"cut at byte {at}, inside {m:02X}", None, data[:at]
    raise KeyError(kind)


def damage_sources(prog) -> dict:
    return PCS.supported_cases() if prog else DC.supported_cases()


@functools.lru_cache(maxsize=None)
def header_damage(prog) -> tuple:
    src = damage_sources(prog)
    bases = PROG_BASES if prog else SEQ_BASES
    plan = PROG_PLAN if prog else SEQ_PLAN
    out = []
    for ki, kind in enumerate(KINDS):
        for j in range(plan[kind]):
            var = PROG_FIELD_ROTATION if prog and kind == "field" else VARIANTS.get(kind)
            want = var[j % len(var)] if var else None
            for turn in range(len(bases)):
                base = bases[(j + ki + turn) % len(bases)]
                if want in ("Hi", "Vi") and "gray" in base and j >= len(FIELDS):   # (a grey frame's factors decide nothing: the second round asks a colour file)
                    continue
                try:
                    how, sub, data = header_damage_of(src[base], kind, np.random.default_rng([DAMAGE_SEED[prog], int(prog), ki, j]), want)
                    break
                except KeyError:
                    continue
            else:
                raise KeyError(f"no base of the list has the field {want}")
            out.append(Damaged(f"{base}:{kind}:{j}", data, kind, base, prog, sub, how))
    assert len(out) == (DAMAGE_PROG if prog else DAMAGE_SEQ) and len({x.name for x in out}) == len(out)
    return tuple(out)


def header_verdict_of(data, S, prog) -> HVerdict:
    try:
        (P.parse if prog else D.parse)(data)
    except D.Unsupported as e:
        return HVerdict("unsupported", e.pos, str(e), None)
    except D.Corrupt as e:
        return HVerdict("corrupt", e.pos, str(e), None)
    return HVerdict("parsed", None, None, M.verdict_of(data, S, prog))


@functools.lru_cache(maxsize=None)
def header_verdict(name, S, prog) -> HVerdict:
    return header_verdict_of(next(x.data for x in header_damage(prog) if x.name == name), S, prog)


def shares(prog) -> dict:
    """kind: [parsed, unsupported, corrupt]"""
    out = {}
    for x in header_damage(prog):
        out.setdefault(x.kind, [0, 0, 0])[("parsed", "unsupported", "corrupt").index(header_verdict(x.name, 256, prog).what)] += 1
    return out


def random_damage(rng):
    """one further damaged header, for the fuzz slice: (description, file, prog)"""
    prog = bool(rng.integers(3) == 0)
    bases = PROG_BASES if prog else SEQ_BASES
    base, kind = bases[int(rng.integers(len(bases)))], KINDS[int(rng.integers(len(KINDS)))]
    how, _, data = header_damage_of(damage_sources(prog)[base], kind, rng)
    return f"odd header {base} {kind}: {how}", data, prog


# ---- the lossless entries ---------------------------------------------------------------------------------------------------------------
V1C_CODE = {"decoded": 0, "refused": -5, "parse": -5, "corrupt": -5, "unsupported": -2}


def shape_of(data, fallback=None):
    """the geometry an output's words need: the file's own where the parse takes it, else the fallback's (a damaged file's base)"""
    try:
        return M._Shape(data)
    except (D.Corrupt, D.Unsupported):
        return M._Shape(fallback)


def transcode_want(data, what, fallback=None):
    """(the whole-image output, the code, the restatement's file or None) of a file whose decode the restatement calls ``what``"""
    import jpgxc_ref as X

    out = X.crop_output(shape_of(data, fallback))
    if what != "decoded":
        return out, V1C_CODE[what], None
    try:
        return out, 0, X.transcode(data, [out])[0]
    except X.Unsupported:
        return out, -2, None


def flip_want(data, what, fallback=None):
    """the same for the whole image mirrored (``flip_h``, a partial last MCU column trimmed); None where the file is narrower than an MCU"""
    import jpgxc_ref as X
    import jpgxf_ref as F

    try:
        out = F.transform_output(shape_of(data, fallback), "flip_h", trim=True)
    except ValueError:
        return None
    if what != "decoded":
        return out, V1C_CODE[what], None
    try:
        return out, 0, F.compose([data], [out])[0]
    except (X.Unsupported, F.Unsupported):
        return out, -2, None


@functools.lru_cache(maxsize=None)
def legal_verdict(name, S):
    """jpgdmg_cases.verdict_of a legal file: ``decoded`` outside the group "complete"; inside it a file whose pad bits -- all ones, which
    a complete code reads as symbols -- make up a further block is ``refused`` for its block count"""
    x = legal_case(name)
    return M.verdict_of(x.data, S, x.prog)


# ---- the fuzz slice -------------------------------------------------------------------------------------------------------------------
# tools/fuzz.py --jpegodd 1 --seed FUZZ_SEED --seconds 10 --cases FUZZ_CASES: what tests/test_gpu_fuzz_jpegodd.py runs on the device (ten
# seconds, or this many cases if they come sooner) and tests/test_jpegdmg_host.py runs through the host builds first
FUZZ_SEED, FUZZ_CASES = 77, 60
