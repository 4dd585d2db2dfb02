"""Damaged JPEG files for the device decoders, shared by the host half (tests/test_jpegdmg_host.py, and the stand-alone sanitizer runs of
the decoders' and the lossless entries' host tests) and the GPU half (tests/test_gpu_jpegdmg.py): INTEGRATION.md section 8 item 6 and
the progressive section say what a damaged scan gives -- only the last pass judges it, the smallest bad bit (of the earliest bad scan)
is reported, a damaged stream that is still a legal one decodes to defined pixels -- and these files hold the kernels to it.

Every file is a small case of jpgdec_cases.supported_cases() or jpgprog_cases.supported_cases() with one damage drawn from a fixed
seed, confined to the entropy-coded bytes of ONE scan (behind the SOS header, in front of the next marker), or one crafted edit of a
header that makes the scan disagree with it.  Nothing is committed: the lists are built on first use and cached, the same bytes on
every machine.  ``verdict`` is the restatement's answer for a file and a subsequence size; every number a test compares is its.

Random kinds: ``bitflip``; ``byte`` (one byte replaced, one time in four by 0xFF, so that the parse decides); ``delete`` and ``insert``
(1-3 bytes); ``swap`` (the contents of two restart segments exchanged, the markers left in place); ``fill`` (the scan replaced by
bytes of its own length: all 00, FF 00 pairs, or random bytes stuffed as an encoder stuffs them; which of the three is fixed per
file, so that each list holds all of them whatever the seed).  Two bases are this module's own (``sources``): a file of 24 MCUs in
restart segments of 5, 5, 5, 5 and 4 with some 390 subsequences at 256 bits, for the exchange of two segments of different lengths
whose refusal two workgroups of the last pass decide, and the end-of-band run file below.  Crafted kinds, sequential: ``dht``
(a table replaced by another file's optimised one: bits that start no code), ``sof`` (one MCU row more, one fewer than the scan holds),
``dri`` (an interval the markers do not serve), ``dcwrap`` (a legal stream whose DC sums leave 16 bits, and the same one block short).
Progressive: ``eobrun`` (an end-of-band run made longer than its segment: the writer's run file of 41 blocks with one bit of the run's length set), ``correction`` (damage inside the correction bits of
w_correction_run's refinement scan), ``dri_changed`` (damage in scans behind a DRI change of w_dri_changed_420), and ``scan_*``: damage
placed in a scan of each of the four kinds.

What the lists give by the restatement (the same at S = 256 and S = 1024; tests/test_jpegdmg_host.py asserts the conditions and prints
these counts as refused by the last pass / decoded / left to the parse, unsupported included):

    sequential, 96 files: 52 refused by the last pass, 34 decoded, 10 left to the parse (8 of them unsupported: a byte that became a
    marker the parse takes for a further scan); 21 of the 52 refusals name a bit other than 0
        bitflip 6 / 14 / 0   byte 8 / 3 / 7   delete 11 / 9 / 0   insert 15 / 3 / 2   swap 2 / 3 / 0   fill 5 / 1 / 0
        dht 1 / 0 / 0        sof 2 / 0 / 0    dri 1 / 0 / 1       dcwrap 1 / 1 / 0
    progressive, 94 files: 52 refused by the last pass, 33 decoded, 9 refused by the parse; 20 of the 52 refusals name a bit other
    than 0
        bitflip 7 / 12 / 1   byte 8 / 7 / 5   delete 15 / 2 / 3   insert 7 / 3 / 0    swap 2 / 2 / 0   fill 3 / 1 / 0
        scan_dc_first 1 / 1 / 0   scan_dc_refine 1 / 1 / 0   scan_ac_first 2 / 0 / 0   scan_ac_refine 1 / 1 / 0
        eobrun 1 / 0 / 0     correction 1 / 2 / 0   dri_changed 3 / 1 / 0
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
import jpgprog_cases as PCS
import jpgprog_ref as P

SEED = 20
SUBSEQ = (256, 1024)
LIMIT = 96                     # files per decoder in the lists the GPU half runs
RANDOM_KINDS = ("bitflip", "byte", "delete", "insert", "swap", "fill")
SCAN_KINDS = ("scan_dc_first", "scan_dc_refine", "scan_ac_first", "scan_ac_refine")  # in the order of jpgprog_ref's kinds

Case = namedtuple("Case", "name data kind base")
Verdict = namedtuple("Verdict", "what bit scan rounds scan_rounds segments subsequences pixels",
                     defaults=(None, None, None, None, None, None, None))
# what: "decoded", "unsupported", "parse" (refused by the parse) or "refused" (by the last pass, with bit, scan and rounds)

# sequential bases: grey, 4:4:4, 4:2:2 and 4:2:0, each with and without restart markers, Annex K and optimised tables
SEQ_BASES = ("noise_q100_gray", "optimised_gray", "dri1_gray", "midrow_444_r7", "optimised_444_smooth", "dri_rows_422", "noise_q100_422",
             "midrow_420_r3", "optimised_420", "dri2_420_noise")
# progressive bases: Pillow's script (successive approximation) and the writer's scripts with Al > 0, with and without restart markers
PROG_BASES = ("pil_gray_q90", "pil_444_q90", "pil_422_q100", "pil_420_rst", "pil_444_rst", "w_al2_420", "w_al3_gray_dri",
              "w_dri_changed_420", "w_correction_run", "w_al2_444")


# ---- where the entropy-coded bytes lie ------------------------------------------------------------------------------------------------
def scan_ranges(data, prog):
    """[(first byte, byte behind the last)] of the entropy-coded bytes of every scan of a file the parse accepts"""
    if prog:
        return [(sc.scan_start, sc.scan_start + sc.scan_len) for sc in P.parse(data).scans]
    s = D.parse(data)
    return [(s.scan_start, s.scan_start + s.scan_len)]


def _markers(data, a, e):
    return [i for i in range(a, e - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


# ---- the damages ----------------------------------------------------------------------------------------------------------------------
def stuffed(raw) -> bytes:
    return bytes(raw).replace(b"\xff", b"\xff\x00")


FILLS = ("zeros", "ff00", "random")


def damage(data, a, e, kind, rng, fill=None, swap=None) -> bytes:
    """``data`` with one damage of a random kind inside [a, e); ``fill``: which of FILLS, ``swap``: which two segments (drawn if None)"""
    b = bytearray(data)
    n = e - a
    if kind == "bitflip":
        b[a + int(rng.integers(n))] ^= 1 << int(rng.integers(8))
    elif kind == "byte":
        i = a + int(rng.integers(n))
        b[i] = 0xFF if rng.integers(4) == 0 and b[i] != 0xFF else (b[i] + 1 + int(rng.integers(255))) & 255
    elif kind == "delete":
        k = min(1 + int(rng.integers(3)), n - 1)
        i = a + int(rng.integers(n - k + 1))
        del b[i:i + k]
    elif kind == "insert":
        k = 1 + int(rng.integers(3))
        i = a + int(rng.integers(n + 1))
        b[i:i] = bytes(rng.integers(0, 256, k, dtype=np.uint8))
    elif kind == "swap":
        m = _markers(data, a, e)
        cut = [a] + [i + 2 for i in m]
        end = m + [e]
        i, j = sorted(int(v) for v in rng.choice(len(cut), 2, replace=False)) if swap is None else swap
        b = bytearray(data[:cut[i]] + data[cut[j]:end[j]] + data[end[i]:cut[j]] + data[cut[i]:end[i]] + data[end[j]:])
    elif kind == "fill":
        mode = FILLS[int(rng.integers(3))] if fill is None else fill
        if mode == "zeros":
            b[a:e] = bytes(n)
        elif mode == "ff00":
            b[a:e] = (b"\xff\x00" * n)[:n - 1] + b"\x00"
        else:
            b[a:e] = (stuffed(rng.integers(0, 256, n, dtype=np.uint8))[:n - 1] + b"\x00")[:n]
    else:
        raise KeyError(kind)
    return bytes(b)


def draw(data, prog, kind, rng, scan=None, **how) -> bytes:
    """one damage of ``kind`` in one scan of ``data`` (``scan``: which; None: drawn), or None where the file has no scan for it"""
    ranges = scan_ranges(data, prog)
    if kind == "swap":
        ok = [i for i, (a, e) in enumerate(ranges) if len(_markers(data, a, e)) >= 2]
    elif kind == "fill":
        ok = [i for i, (a, e) in enumerate(ranges) if not _markers(data, a, e)]
    else:
        ok = list(range(len(ranges)))
    if scan is not None:
        ok = [i for i in ok if i == scan]
    if not ok:
        return None
    a, e = ranges[ok[int(rng.integers(len(ok)))]]
    return damage(data, a, e, kind, rng, **how)


def _rng(*key):
    return np.random.default_rng([SEED, *key])


# ---- crafted edits ----------------------------------------------------------------------------------------------------------------------
def dht_table(data, tc_th) -> bytes:
    """the 17 + n bytes of table ``tc_th`` of a file's DHT segments"""
    for m, a, e in DC.header_segments(data):
        i = a + 4
        while m == 0xC4 and i < e:
            n = sum(data[i + 1:i + 17])
            if data[i] == tc_th:
                return data[i:i + 17 + n]
            i += 17 + n
    raise KeyError(tc_th)


def with_dht_table(data, table) -> bytes:
    """the file with the table of ``table``'s class and number replaced (its segment rewritten at its new length)"""
    for m, a, e in DC.header_segments(data):
        i = a + 4
        while m == 0xC4 and i < e:
            n = sum(data[i + 1:i + 17])
            if data[i] == table[0]:
                return data[:a] + DC.segment(0xC4, data[a + 4:i] + table + data[i + 17 + n:e]) + data[e:]
            i += 17 + n
    raise KeyError(table[0])


def edit_sof_size(data, height=None, width=None) -> bytes:
    m, a, e = next(s for s in DC.header_segments(data) if s[0] in (0xC0, 0xC1, 0xC2))
    b = bytearray(data)
    if height is not None:
        b[a + 5:a + 7] = struct.pack(">H", height)
    if width is not None:
        b[a + 7:a + 9] = struct.pack(">H", width)
    return bytes(b)


def eobrun_file() -> bytes:
    """The writer's run file at 41 blocks: flat but for one coefficient of the last block, so that the first AC scan is one end-of-band
    run of 40 blocks -- EOB5 and the five bits 01000 -- and the last block's symbol."""
    g = PCS._G(8, 8 * 41, 1)
    zz = np.zeros((g.nblocks, 64), np.int16)
    zz[:, 0] = 3
    zz[-1, 5] = -2
    q16 = np.full(64, 16, np.int64)
    return PCS.progressive(zz, g, [q16, q16], PCS.full([0], 1))


# ---- the lists ------------------------------------------------------------------------------------------------------------------------
LONG_DRI = "dri5_420_noise_64x96"   # 24 MCUs in segments of 5, 5, 5, 5 and 4; some 390 subsequences at 256 bits
CORRECTION_HEAD = 4                 # bytes of w_correction_run's last scan that hold its one symbol and the run's length


@functools.lru_cache(maxsize=None)
def sources(prog) -> dict:
    """the sound files the cases are made of: the supported cases, and the two bases this module writes itself"""
    if prog:
        return {**PCS.supported_cases(), "w_eobrun_40": eobrun_file()}
    return {**DC.supported_cases(), LONG_DRI: R.encode(PC.noise(64, 96, 3, 70), 100, "420", 5)}


# per base: how many files of each random kind
_SEQ_PLAN = dict(bitflip=2, byte=2, delete=2, insert=2)
_PROG_PLAN = dict(bitflip=2, byte=2, delete=2, insert=1)


def _random_cases(bases, cases, prog, plan, extra):
    out = []
    for bi, base in enumerate(bases):
        data = cases[base]
        for ki, kind in enumerate(RANDOM_KINDS):
            for k in range(plan.get(kind, 0) + extra.get((base, kind), 0)):
                d = draw(data, prog, kind, _rng(int(prog), bi, ki, k))
                if d is not None:
                    out.append(Case(f"{base}:{kind}:{k}", d, kind, base))
    return out


@functools.lru_cache(maxsize=None)
def sequential_cases() -> tuple:
    c = DC.supported_cases()
    extra = {(b, "swap"): 1 for b in ("midrow_444_r7", "dri_rows_422", "midrow_420_r3", "dri2_420_noise")}
    extra.update({("optimised_gray", "byte"): -1, ("optimised_420", "byte"): -1})
    out = _random_cases(SEQ_BASES, c, False, _SEQ_PLAN, extra)
    # every fill, each on a fixed base: FF 00 pairs -- an all-ones stream, every lane of every workgroup meets bits that start no
    # code -- on the file with the longest scan, which still has some 390 subsequences at 256 bits once the pairs are unstuffed: two
    # workgroups of the last pass
    for k, (base, fill) in enumerate((("noise_q100_444", "ff00"), ("noise_q100_gray", "random"), ("optimised_444_smooth", "zeros"),
                                      ("noise_q100_422", "ff00"), ("optimised_420", "random"))):
        out.append(Case(f"{base}:fill:{fill}", draw(c[base], False, "fill", _rng(5, k), fill=fill), "fill", base))
    # two restart segments of different lengths exchanged, the second of them in the last pass's second workgroup at 256 bits: both are
    # refused for their block counts, and the smaller bit -- not 0 -- is decided between workgroups
    long = sources(False)[LONG_DRI]
    out.append(Case(f"{LONG_DRI}:swap:short_last", draw(long, False, "swap", _rng(6), swap=(1, 4)), "swap", LONG_DRI))
    # a scan of one block: 32 bytes of 00 are one whole block of Annex K codes and the start of a second, a legal stream
    tiny = c["size_8x8_gray"]
    a, e = scan_ranges(tiny, False)[0]
    out.append(Case("size_8x8_gray:fill:zeros", tiny[:a] + bytes(e - a) + tiny[e:], "fill", "size_8x8_gray"))
    # crafted: another file's optimised table; one MCU row more and fewer; a restart interval the markers do not serve
    annexk = c["size_17x17_420"]
    out.append(Case("size_17x17_420:dht:ac0", with_dht_table(annexk, dht_table(c["optimised_420"], 0x10)), "dht", "size_17x17_420"))
    s = D.parse(c["optimised_420"])
    out.append(Case("optimised_420:sof:row_more", edit_sof_size(c["optimised_420"], height=s.h - 16), "sof", "optimised_420"))
    out.append(Case("optimised_420:sof:row_fewer", edit_sof_size(c["optimised_420"], height=s.h + 16), "sof", "optimised_420"))
    out.append(Case("dri_rows_422:dri:larger", DC.edit_dri(c["dri_rows_422"], 6), "dri", "dri_rows_422"))   # 25 MCUs: five segments still
    out.append(Case("dri_rows_422:dri:smaller", DC.edit_dri(c["dri_rows_422"], 4), "dri", "dri_rows_422"))  # seven segments: the parse's
    # a legal stream whose DC sums leave 16 bits: every block the Annex K codes of a difference of +2047 and EOB (FF 7F FA, stuffed),
    # 96 blocks of them -- the sum wraps as INTEGRATION.md section 8 item 7 says and decodes to those pixels --, and 95: one too few
    grey = c["noise_q100_gray"]
    a, e = scan_ranges(grey, False)[0]
    n = D.parse(grey).nblocks
    out.append(Case("noise_q100_gray:dcwrap:whole", grey[:a] + b"\xff\x00\x7f\xfa" * n + grey[e:], "dcwrap", "noise_q100_gray"))
    out.append(Case("noise_q100_gray:dcwrap:short", grey[:a] + b"\xff\x00\x7f\xfa" * (n - 1) + grey[e:], "dcwrap", "noise_q100_gray"))
    assert len(out) <= LIMIT and len({x.name for x in out}) == len(out)
    return tuple(out)


def _first_scan_of_kind(data, kind):
    return next(i for i, sc in enumerate(P.parse(data).scans) if sc.kind == kind)


@functools.lru_cache(maxsize=None)
def progressive_cases() -> tuple:
    c = PCS.supported_cases()
    extra = {(b, "swap"): 2 for b in ("pil_420_rst", "pil_444_rst")}
    out = _random_cases(PROG_BASES, c, True, _PROG_PLAN, extra)
    for k, (base, fill) in enumerate((("pil_gray_q90", "zeros"), ("pil_444_q90", "ff00"), ("w_al2_420", "random"), ("w_al2_444", "ff00"))):
        # (the zeros go into the DC refinement scan, where any bits are a legal stream: the fill that decodes)
        scan = _first_scan_of_kind(c[base], 1) if fill == "zeros" else None
        out.append(Case(f"{base}:fill:{fill}", draw(c[base], True, "fill", _rng(5, k), scan=scan, fill=fill), "fill", base))
    # damage placed in a scan of each kind
    for kind, name in enumerate(SCAN_KINDS):
        for k, (base, how) in enumerate((("pil_420_q90", "delete"), ("w_al2_444", "bitflip"))):
            d = draw(c[base], True, how, _rng(2, kind, k), scan=_first_scan_of_kind(c[base], kind))
            out.append(Case(f"{base}:{name}:{k}", d, name, base))
    # an end-of-band run past the end of its segment: the run's length 40 -> 56 of 41 blocks
    run = eobrun_file()
    a, e = scan_ranges(run, True)[1]
    sc = P.parse(run).scans[1]
    ln = sc.ac.lut[int.from_bytes(run[a:a + 2], "big")] >> 8     # the EOB5 symbol's length: the run's bits lie behind it
    assert sc.ac.lut[int.from_bytes(run[a:a + 2], "big")] & 255 == 0x50
    b = bytearray(run)
    b[a + (ln >> 3)] ^= 0x80 >> (ln & 7)
    out.append(Case("w_eobrun_40:eobrun:past_segment", bytes(b), "eobrun", "w_eobrun_40"))
    # the correction bits of w_correction_run's refinement scan (its last): behind the scan's first CORRECTION_HEAD bytes -- the one
    # end-of-band symbol and its run's length -- every bit is a correction bit; and scans behind a DRI change
    a, e = scan_ranges(c["w_correction_run"], True)[3]
    for k in range(3):
        d = damage(c["w_correction_run"], a + CORRECTION_HEAD, e, "bitflip" if k < 2 else "delete", _rng(3, k))
        out.append(Case(f"w_correction_run:correction:{k}", d, "correction", "w_correction_run"))
    for k, scan in enumerate((1, 4, 6, 7)):
        d = draw(c["w_dri_changed_420"], True, ("delete", "bitflip", "insert", "byte")[k], _rng(4, k), scan=scan)
        out.append(Case(f"w_dri_changed_420:dri_changed:{k}", d, "dri_changed", "w_dri_changed_420"))
    assert len(out) <= LIMIT and len({x.name for x in out}) == len(out)
    return tuple(out)


def cases(prog) -> tuple:
    return progressive_cases() if prog else sequential_cases()


def longer_draw(prog, n, seed=1) -> list:
    """``n`` further files of the same generator (random kinds only), for the host half alone"""
    src = PCS.supported_cases() if prog else DC.supported_cases()
    bases = PROG_BASES if prog else SEQ_BASES
    out, k = [], 0
    while len(out) < n:
        rng = _rng(9, int(prog), seed, k)
        base, kind = bases[int(rng.integers(len(bases)))], RANDOM_KINDS[int(rng.integers(len(RANDOM_KINDS)))]
        d = draw(src[base], prog, kind, rng)
        if d is not None:
            out.append(Case(f"{base}:{kind}:x{k}", d, kind, base))
        k += 1
    return out


# ---- the restatement's verdict --------------------------------------------------------------------------------------------------------
def _bit_of(e):
    return int(str(e).split("bit ")[1].split()[0])


def verdict_of(data, S, prog, check=False) -> Verdict:
    """What the contract says of ``data`` at subsequence size ``S``.  ``check``: on a file that decodes, the plain decoder must agree
    with the iteration (coefficients, and the entry states wherever it passes a subsequence's first bit)."""
    try:
        s = (P.parse if prog else D.parse)(data)
    except D.Unsupported:
        return Verdict("unsupported")
    except D.Corrupt:
        return Verdict("parse")
    if not prog:
        st = D.Stream(s, S)
        entry, counts, rounds = D.synchronise(st)
        assert rounds <= len(st.subs) + 1
        try:
            coef = D.coefficients(st, entry, counts)
        except D.Corrupt as e:
            return Verdict("refused", _bit_of(e), 0, rounds, [rounds], s.nseg, len(st.subs))
        if check:
            plain, states = D.sequential(st)
            assert np.array_equal(plain, coef) and all(a is None or a == b for a, b in zip(states, entry))
        return Verdict("decoded", None, None, rounds, [rounds], s.nseg, len(st.subs), D.pixels(s, D.dc_values(s, coef)))
    coef = np.zeros((s.nblocks, 64), np.int16)
    scan_rounds, nseg, nsub = [], 0, 0
    for n, sc in enumerate(s.scans):
        st = P.Stream(s, sc, S)
        before = coef.copy() if check else None
        entry, counts, rounds = P.synchronise(st, coef)
        assert rounds <= len(st.subs) + 1
        scan_rounds.append(rounds)
        nseg, nsub = nseg + sc.nseg, nsub + len(st.subs)
        try:
            P.last_pass(st, coef, entry, counts)
        except D.Corrupt as e:
            return Verdict("refused", _bit_of(e), n, sum(scan_rounds), scan_rounds)
        if check:
            states = P.plain_scan(st, before)
            assert np.array_equal(before, coef) and all(a is None or a == b for a, b in zip(states, entry)), n
    return Verdict("decoded", None, None, sum(scan_rounds), scan_rounds, nseg, nsub, P.pixels(s, coef))


@functools.lru_cache(maxsize=None)
def verdict(name, S, prog) -> Verdict:
    """``verdict_of`` a file of the lists, computed once"""
    return verdict_of(next(x.data for x in cases(prog) if x.name == name), S, prog)


def shares(prog, S) -> dict:
    """kind: [refused by the last pass, decoded, refused by the parse or unsupported]"""
    out = {}
    for x in cases(prog):
        v = verdict(x.name, S, prog).what
        out.setdefault(x.kind, [0, 0, 0])[("refused", "decoded").index(v) if v in ("refused", "decoded") else 2] += 1
    return out


# ---- the lossless entries on the sequential list --------------------------------------------------------------------------------------
V1C_OK, V1C_E_UNSUPPORTED, V1C_E_CORRUPT = 0, -2, -5


def base_of(x) -> bytes:
    """the sound file a sequential case was made of"""
    return sources(False)[x.base]


class _Shape:
    """what an output's geometry needs of a source, by the parse alone: a refused source has no coefficients"""

    def __init__(self, data):
        s = self.info = D.parse(data)
        self.mw, self.mh = 8 * s.hs, 8 * s.vs


def shape_of(x):
    """the case's geometry for an output's words: the file's own where the parse takes it, else its base's"""
    try:
        return _Shape(x.data)
    except (D.Corrupt, D.Unsupported):
        return _Shape(base_of(x))


@functools.lru_cache(maxsize=None)
def transcode_want(name):
    """(the whole-image output of the case as jpgxc_ref's crop_output words it, the code, the restatement's file or None): a damaged
    source that decodes gives the restatement's bytes, or the out-of-range refusal the restatement gives"""
    import jpgxc_ref as X

    x = next(c for c in sequential_cases() if c.name == name)
    out = X.crop_output(shape_of(x))
    v = verdict(name, 256, False)
    if v.what != "decoded":
        return out, V1C_E_UNSUPPORTED if v.what == "unsupported" else V1C_E_CORRUPT, None
    try:
        return out, V1C_OK, X.transcode(x.data, [out])[0]
    except X.Unsupported:
        return out, V1C_E_UNSUPPORTED, None


@functools.lru_cache(maxsize=None)
def join_want(name):
    """The case as the SECOND source of a join behind its sound base: (the output, the code, the restatement's file or None), or None
    where the two do not make a join (a crafted height).  The damaged source's report is source 1's."""
    import jpgxc_ref as X
    import jpgxf_ref as F

    x = next(c for c in sequential_cases() if c.name == name)
    left = X.Source(base_of(x))
    try:
        out = F.join_output(left, shape_of(x), trim=True)
    except ValueError:
        return None
    v = verdict(name, 256, False)
    if v.what != "decoded":
        return out, V1C_E_UNSUPPORTED if v.what == "unsupported" else V1C_E_CORRUPT, None
    try:
        return out, V1C_OK, F.compose([left, x.data], [out])[0]
    except (X.Unsupported, F.Unsupported):
        return out, V1C_E_UNSUPPORTED, None


# ---- batches of the sequential list ---------------------------------------------------------------------------------------------------
# max_workspace_bytes of the "chunked" batch per subsequence size: the smallest budget under which a damaged file opens a chunk and
# another closes one with three to five chunks, by the product's own layout (tests/test_jpegdmg_host.py computes it with the batch's
# host build and asserts these numbers)
CHUNK_BUDGET = {256: 122416, 1024: 114480}
# ... and where the chunks then end, as indices into the batch's files (behind the last file of each chunk)
CHUNK_ENDS = {256: [3, 5, 8, 10, 12], 1024: [3, 5, 8, 10, 12]}


def batches():
    """name: [(the damaged case's name or None, the sound case's name or None, the file)] -- the three batches of twelve that the host
    half and the GPU half run: damaged files first, in the middle and last among sound ones; every file damaged; and one for a budget
    under which a damaged file opens a chunk and another closes one (CHUNK_BUDGET)"""
    cases = {x.name: x for x in sequential_cases()}
    kind = lambda n: verdict(n, 256, False).what
    refused = [n for n in cases if kind(n) == "refused"]
    decoded = [n for n in cases if kind(n) == "decoded"]
    parse = [n for n in cases if kind(n) in ("parse", "unsupported")]
    sound = ["size_17x17_420", "dri1_444", "optimised_gray", "midrow_420_r3", "size_15x33_422", "noise_q100_422", "flat_gray_200"]
    ok = lambda n: (None, n, sources(False)[n])
    dm = lambda n: (n, None, cases[n].data)
    mixed = [dm(refused[0]), ok(sound[0]), ok(sound[1]), dm(refused[7]), dm(decoded[0]), ok(sound[2]), dm(parse[0]), ok(sound[3]),
             dm(refused[15]), ok(sound[4]), ok(sound[5]), dm(refused[23])]
    damaged = [dm(n) for n in refused[1:12:2] + decoded[1:8:2] + parse[1:3]]
    chunked = [dm(refused[2]), ok(sound[0]), dm(refused[9]), dm(refused[4]), ok(sound[6]), ok(sound[1]), dm(decoded[2]), ok(sound[3]),
               dm(refused[30]), dm(refused[6]), ok(sound[2]), dm(refused[11])]
    return {"mixed": mixed, "all_damaged": damaged, "chunked": chunked}


def batch_wants(files, S):
    return [verdict(dmg, S, False) if dmg else verdict_of(data, S, False) for dmg, sound, data in files]


def chunk_ends(ws, budget):
    """files in order while their sum stays within the budget; a file above it is a chunk of its own"""
    ends, total = [], 0
    for i, w in enumerate(ws):
        if total and total + w > budget:
            ends.append(i)
            total = 0
        total += w
    return ends + [len(ws)]


def batch_rounds_of(wants, ends):
    """what the per-file rounds imply: every chunk takes the rounds of its slowest file"""
    starts = [0] + ends[:-1]
    return sum(max(w.rounds for w in wants[a:e]) for a, e in zip(starts, ends))



def lossless_subset() -> list:
    """the files of the sequential list the GPU half sends through v1c_jpeg_transcode and v1c_jpeg_compose: every sixth, 16 files;
    the file whose DC sums wrap (it decodes, and its DC is outside what the encoder's tables code); and the two whose refusal two
    workgroups of the last pass decide"""
    cases = list(sequential_cases())
    also = ("noise_q100_gray:dcwrap:whole", "noise_q100_444:fill:ff00", LONG_DRI + ":swap:short_last")
    return cases[::6] + [x for x in cases if x.name in also and x not in cases[::6]]


# ---- the fuzz slice -------------------------------------------------------------------------------------------------------------------
# tools/fuzz.py --jpegdmg 1 --seed FUZZ_SEED --cases FUZZ_CASES: what tests/test_gpu_fuzz_jpegdmg.py runs on the device and
# tests/test_jpegdmg_host.py runs through the host builds first.  The seed is picked on the CPU so that the restatement alone refuses at
# least 10 of the cases in the last pass and decodes at least 5.
FUZZ_SEED, FUZZ_CASES = 411, 40
