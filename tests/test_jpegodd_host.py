"""Odd legal files and damaged headers without a GPU (tests/jpgodd_cases.py): what the two lists hold; the restatements against Pillow
on them; the product's host builds -- tests/host_jpegdec, tests/host_jpegdec_batch, tests/host_jpegdec_prog, tests/host_jpegxf (which
has tests/host_jpegxc) -- against the restatements value for value; the product's parse-only entries against the restatements' class
and error position on every damaged header; and both lists through the stand-alone sanitizer programs of the host builds.
tests/test_gpu_jpegodd.py then holds the kernels to the same values on exactly these files."""
import ctypes as C
import io
import subprocess

import numpy as np
import pytest

import jpgdec_ref as D
import jpgodd_cases as O
import jpgprog_ref as P
import jpgxc_ref as X
import test_jpegdec_batch_host as TB
import test_jpegdec_host as TD
import test_jpegdmg_host as TM
import test_jpegprog_host as TP
import test_jpegxc_host as TX
import test_jpegxf_host as TF

LEGAL = O.legal()
SEQ = [x for x in LEGAL if not x.prog]
PROG = [x for x in LEGAL if x.prog]
HOST_CODE = {"parsed": 0, "unsupported": 1, "corrupt": 2}
ABI_CODE = {"parsed": 0, "unsupported": -2, "corrupt": -5}

# Damaged headers on which Pillow 12.2 (libjpeg-turbo 3.1) and the restatement do not agree on whether the file decodes, counted on the
# CPU; both sides are deterministic.  libjpeg is the more forgiving reader: it takes a missing DHT for the Annex K tables, skips to the
# next marker where a length is wrong, decodes a scan whose Ss / Se / Ah / Al bytes are not a baseline scan's and stops with a warning
# where the scan is short, a code is missing or a restart marker out of turn, and takes a progressive script as it comes; the product
# refuses all of these (15 + 14 files).  The one file of each list that the restatement decodes and Pillow refuses is a grey frame whose
# vertical sampling factor became 10 or 14: T.81 allows 1 ... 4 and libjpeg refuses the frame, while the parse here ignores the factors
# of a frame of one component; the test asserts that these are the only such files and prints every file
# with both reasons.
PILLOW_DISAGREES = {False: 16, True: 15}


def _pillow(data):
    from PIL import Image

    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])


@pytest.fixture(scope="module")
def emul_seq(tmp_path_factory):
    lib = TM._build(TD.HARNESS, tmp_path_factory.mktemp("odd_jpegdec") / "libjpegdec_emul.so")
    vp, u32 = C.c_void_p, C.c_uint32
    lib.jdec_emul_info.argtypes = [C.c_char_p, C.c_uint64, vp]
    lib.jdec_emul_decode.argtypes = [C.c_char_p, C.c_uint64, u32, C.c_int, vp, vp, vp, u32, vp, vp]
    return lib


@pytest.fixture(scope="module")
def emul_prog(tmp_path_factory):
    lib = TM._build(TP.HARNESS, tmp_path_factory.mktemp("odd_jpegprog") / "libjpegprog_emul.so")
    vp, u32 = C.c_void_p, C.c_uint32
    lib.jprog_emul_info.argtypes = [C.c_char_p, C.c_uint64, vp]
    lib.jprog_emul_decode.argtypes = [C.c_char_p, C.c_uint64, u32, C.c_int, vp, u32, vp, vp, u32, vp, vp, vp, vp]
    return lib


@pytest.fixture(scope="module")
def emul_batch(tmp_path_factory):
    return TB._build(tmp_path_factory.mktemp("odd_jpegdec_batch") / "libjpegdec_batch_emul.so")


@pytest.fixture(scope="module")
def emul_xf(tmp_path_factory):
    lib = TM._build(TF.HARNESS, tmp_path_factory.mktemp("odd_jpegxf") / "libjpegxf_emul.so")
    lib.jxc_emul_transcode.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.jxf_emul_compose.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
                                     C.c_void_p]
    return lib


# ---- the legal list -------------------------------------------------------------------------------------------------------------------
def _named_tables(x):
    """the (BITS, HUFFVAL) of every table a scan of the file names"""
    if x.prog:
        out = []
        for sc in P.parse(x.data).scans:
            out += [(h.bits, h.vals) for h in (sc.jdc if sc.kind == P.DC_FIRST else [sc.ac] if sc.kind >= P.AC_FIRST else [])]
        return out
    s = D.parse(x.data)
    return [(s.dc[t].bits, s.dc[t].vals) for t in s.td] + [(s.ac[t].bits, s.ac[t].vals) for t in s.ta]


def test_legal_list_holds_what_it_is_for():
    """every tag in at least two files of different sampling, the group "complete" exactly a quarter, and the tags true of the bytes"""
    assert len(LEGAL) <= 64 and len(SEQ) == O.LEGAL_SEQ and len(PROG) == O.LEGAL_PROG <= 16
    for tag in O.TAGS:
        assert len({x.sampling for x in LEGAL if tag in x.tags}) >= 2, tag
    for tag in O.GREY_TAGS:
        assert sum(tag in x.tags for x in LEGAL) >= 2, tag
    for tag in ("random", "long", "unused_dc", "unused_ac", "complete", "slots"):     # ... and the progressive files draw these too
        assert len({x.sampling for x in PROG if tag in x.tags}) >= 2, tag
    assert 4 * sum(x.group == "complete" for x in LEGAL) == len(LEGAL)
    assert {x.sampling for x in LEGAL if x.group == "complete"} == set(O.SAMPLINGS)
    slots_dc, slots_ac, slots_q, sizes = set(), set(), set(), set()
    for x in LEGAL:
        tabs = _named_tables(x)
        sums = [O.kraft(t) for t in tabs]
        assert ("complete" in x.tags) == (x.group == "complete") == (max(sums) == 1 << 16), x.name
        assert max(sums) <= 1 << 16
        if "long" in x.tags:                                # no code of up to kLutBits bits: the lookup is empty
            assert any(sum(b) > 1 and not any(b[:O.LUT_BITS]) for b, _ in tabs), x.name
        if "one1" in x.tags:
            assert any(list(b) == [1] + [0] * 15 for b, _ in tabs), x.name
        if "one16" in x.tags:
            assert any(list(b) == [0] * 15 + [1] for b, _ in tabs), x.name
        if "unused_dc" in x.tags:
            assert any(len(v) <= 16 and max(v) >= 12 for _, v in tabs), x.name
        if "unused_ac" in x.tags:
            assert any(any(v & 15 >= 11 for v in vals) for _, vals in tabs), x.name
        s = (P if x.prog else D).parse(x.data)
        sizes.add((s.h, s.w))
        assert 1 <= s.h <= 48 and 1 <= s.w <= 48 and (s.nc == 1) == (x.sampling == "gray")
        if x.prog:
            continue
        assert len(set(s.td)) == len(set(s.ta)) == s.nc and "slots" in x.tags, x.name    # every component its own tables
        assert ("random" in x.tags) <= any(sum(b) >= 1 and any(b[:O.LUT_BITS]) and O.kraft((b, v)) < 1 << 16 for b, v in tabs), x.name
        slots_dc |= set(s.td)
        slots_ac |= set(s.ta)
        slots_q |= set(s.tq)
        segs = O.segments(x.data)
        sof = next(x.data[a:e] for m, a, e in segs if m in (0xC0, 0xC1))
        ids = [sof[10 + 3 * i] for i in range(s.nc)]
        assert ("ids" in x.tags) == (ids != [1, 2, 3][:s.nc]) and len(set(ids)) == s.nc, x.name
        assert ("dqt16" in x.tags) == (sof[1] == 0xC1), x.name                          # SOF1 whenever a table is 16-bit
        assert "tq_slots" in x.tags and [sof[12 + 3 * i] for i in range(s.nc)] == s.tq and (s.nc == 1 or s.tq[0] != s.tq[1]), x.name
        dqt = [(x.data[i] >> 4, x.data[i] & 15, x.data[i + 1:i + 1 + 64 * ((x.data[i] >> 4) + 1)]) for m, a, e in segs if m == 0xDB
               for i in _dqt_heads(x.data, a, e)]
        assert ("dqt_redefined" in x.tags) == (len({t for _, t, _ in dqt}) < len(dqt)), x.name
        assert ("dqt8" in x.tags) == any(pq == 0 and s.tq.count(t) and i == max(j for j, d in enumerate(dqt) if d[1] == t)
                                         for i, (pq, t, _) in enumerate(dqt)), x.name     # (a table in force with 8-bit entries)
        assert ("dqt16" in x.tags) == any(pq == 1 for pq, t, body in dqt), x.name
        if "dqt16_high" in x.tags:                          # an entry above 255 that some block's coefficient meets
            r = D.decode(x.data, check=False)
            assert (np.abs(r.coef[::s.bpm, 1:]).max(axis=0) * (s.q[s.tq[0]][O.R.ZIGZAG[1:]] > 255)).any(), x.name
        assert ("grey_2x2" in x.tags, "grey_1x2" in x.tags) == (s.nc == 1 and sof[11] == 0x22, s.nc == 1 and sof[11] == 0x12), x.name
        assert any(m == 0xE0 and x.data[a + 4:a + 8] == b"JFIF" for m, a, e in segs), x.name
        order = [m for m, a, e in segs]
        assert ("dri_first" in x.tags) == (order[0] == 0xDD), x.name
        assert ("dht_first" in x.tags) == (order.index(0xC4) < min(order.index(0xDB), order.index(sof[1]))), x.name
        assert ("dqt_last" in x.tags) == (order[-2] == 0xDB), x.name
        assert ("two_dri" in x.tags) == (order.count(0xDD) == 2), x.name
        assert ("dri_large" in x.tags) == (s.restart > s.nmcu), x.name
        assert ("app65535" in x.tags) == any(e - a - 2 == 65535 for m, a, e in segs) and ("com2" in x.tags) == any(e - a == 4 for m, a, e in segs)
        assert ("fill_eoi" in x.tags) == x.data.endswith(b"\xff\xff\xff\xff\xd9"), x.name
        assert ("fill" in x.tags) == (x.data[2:4] == b"\xff\xff"), x.name
        scan = x.data[s.scan_start:s.scan_start + s.scan_len]
        assert ("fill_rst" in x.tags) == any(scan[i:i + 2] == b"\xff\xff" and 0xD0 <= scan[i + 2] <= 0xD7 for i in range(len(scan) - 2)), x.name
        if "decoy_same_segment" in x.tags or "decoy_two_segments" in x.tags:
            ids = [x.data[i] for m, a, e in segs if m == 0xC4 for i in _dht_heads(x.data, a, e)]
            per_seg = [[x.data[i] for i in _dht_heads(x.data, a, e)] for m, a, e in segs if m == 0xC4]
            assert len(ids) > len(set(ids)), x.name
            assert ("decoy_same_segment" in x.tags) == any(len(p) > len(set(p)) for p in per_seg), x.name
        if "unnamed_table" in x.tags:
            defined = {x.data[i] for m, a, e in segs if m == 0xC4 for i in _dht_heads(x.data, a, e)}
            assert defined - ({t for t in s.td} | {0x10 | t for t in s.ta}), x.name
    assert slots_dc == slots_ac == slots_q == {0, 1, 2, 3}
    assert (1, 1) in sizes and (48, 48) in sizes and len(sizes) >= 6


def _dqt_heads(data, a, e):
    i = a + 4
    while i < e:
        yield i
        i += 1 + 64 * ((data[i] >> 4) + 1)


def _dht_heads(data, a, e):
    i = a + 4
    while i < e:
        yield i
        i += 17 + sum(data[i + 1:i + 17])


def test_restatement_against_pillow_on_the_legal_list():
    """outside the group "complete": Pillow opens every file and the pixels are equal; the restatement's plain decoder agrees with its
    iteration on every file it decodes.  Inside the group Pillow may refuse (libjpeg takes no code of all ones); where it does not,
    the pixels are equal too.  How many of the group it refuses is printed."""
    refused = ours = 0
    for x in LEGAL:
        v = O.legal_verdict(x.name, 256)
        assert v.what == "decoded" or (v.what == "refused" and x.group == "complete"), (x.name, v.what)
        if v.what == "decoded":
            assert O.M.verdict_of(x.data, 256, x.prog, check=True).what == "decoded"
            assert np.array_equal(O.legal_verdict(x.name, 1024).pixels, v.pixels), x.name
        else:
            ours += 1
        try:
            got = _pillow(x.data)
        except OSError as e:
            assert x.group == "complete", (x.name, e)
            refused += 1
            continue
        if v.what == "decoded":
            assert np.array_equal(got, v.pixels), x.name
    n = sum(x.group == "complete" for x in LEGAL)
    print(f"group complete: Pillow refuses {refused} of {n}; the restatement refuses {ours} of {n} for their block counts (pad bits read as blocks)")


@pytest.mark.parametrize("S", O.SUBSEQ)
def test_sequential_host_build_equals_restatement_on_the_legal_list(emul_seq, emul_batch, S):
    """geometry, coefficients, entry states, block counts, segments, subsequences, rounds and pixels; a refused file's bit and rounds;
    then the whole list as one batch, every file the single call's"""
    for x in SEQ:
        v = O.legal_verdict(x.name, S)
        assert not TM.seq_differences(emul_seq, x.data, S, v), x.name
        s = D.parse(x.data)
        rc, info = TD._emul_info(emul_seq, x.data)
        assert rc == 0 and info.tolist() == [s.h, s.w, s.nc, s.hs, s.vs, s.restart, s.nseg, s.nblocks], x.name
        if v.what != "decoded":
            continue
        want = D.decode(x.data, S, check=False)
        rc, coef, states, counts, report, px = TD._emul_decode(emul_seq, x.data, S)
        assert rc == 0 and np.array_equal(coef, want.coef), x.name
        assert [tuple(t) for t in states.tolist()] == want.entry and counts.tolist() == want.counts, x.name
    res, (rounds, chunks) = TB.run_batch(emul_batch, [x.data for x in SEQ], S)
    wants = [O.legal_verdict(x.name, S) for x in SEQ]
    for x, r, v in zip(SEQ, res, wants):
        assert r.status == TM.CODE[v.what] and r.report[:3] == [v.segments, v.subsequences, v.rounds], x.name
        assert np.array_equal(r.pixels, v.pixels) if v.what == "decoded" else r.report[3] == v.bit, x.name
    assert chunks == 1 and rounds == max(v.rounds for v in wants)


@pytest.mark.parametrize("S", O.SUBSEQ)
def test_progressive_host_build_equals_restatement_on_the_legal_list(emul_prog, S):
    for x in PROG:
        v = O.legal_verdict(x.name, S)
        assert not TM.prog_differences(emul_prog, x.data, S, v), x.name
        if v.what != "decoded":
            continue
        ref = P.decode(x.data, S, check=False)
        rc, after, states, counts, rounds, nsub, report, px = TP._emul_decode(emul_prog, x.data, S)
        assert rc == 0 and np.array_equal(after[-1], ref.coef), x.name
        assert [tuple(int(t) for t in s) for s in states] == [e for es in ref.entries for e in es], x.name
        assert list(counts) == [c for cs in ref.counts for c in cs] and list(nsub) == [len(e) for e in ref.entries], x.name


@pytest.mark.parametrize("S", O.SUBSEQ)
def test_lossless_host_builds_equal_restatement_on_the_legal_list(emul_xf, S):
    """the whole image through the transcoder and mirrored through the composer: the restatement's bytes; read back, the transcoded
    file has the source's coefficients and tables"""
    flips = 0
    for x in SEQ:
        v = O.legal_verdict(x.name, S)
        out, code, want = O.transcode_want(x.data, v.what)
        rc, made = TX.run_emul(emul_xf, x.data, [out], S, O.shape_of(x.data))
        assert rc == code and (code != 0 or made[0][1] == want), (x.name, rc, code)
        if code == 0:
            a, b = D.decode(x.data, S, check=False), D.decode(want, S, check=False)
            assert np.array_equal(D.dc_values(a.info, a.coef), D.dc_values(b.info, b.coef)), x.name
            assert all(np.array_equal(a.info.q[a.info.tq[c]], b.info.q[b.info.tq[c]]) for c in range(a.info.nc)), x.name
            assert np.array_equal(a.pixels, b.pixels), x.name
        f = O.flip_want(x.data, v.what)
        if f is not None:
            out, code, want = f
            rc, made, _ = TF.run_emul(emul_xf, [x.data], [out], S)
            assert rc == code and (code != 0 or made[0][1] == want), (x.name, rc, code)
            flips += code == 0
    assert flips >= 24


# ---- the damage lists -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prog", TM.DECODERS)
def test_damage_lists_hold_every_kind_and_every_verdict(prog):
    """by the restatement alone; the counts are printed: the case module's docstring quotes them"""
    cases = O.header_damage(prog)
    sh = O.shares(prog)
    total = [sum(v[i] for v in sh.values()) for i in range(3)]
    print(f"{'progressive' if prog else 'sequential'}: {len(cases)} files, parsed / unsupported / corrupt {total};",
          "  ".join(f"{k} {v[0]}/{v[1]}/{v[2]}" for k, v in sh.items()))
    inner = [O.header_verdict(x.name, 256, prog).inner.what for x in cases if O.header_verdict(x.name, 256, prog).what == "parsed"]
    print("    of the parsed files:", {w: inner.count(w) for w in sorted(set(inner))})
    assert len(cases) <= (48 if prog else 96) and set(sh) == set(O.KINDS)
    # every variant the kinds name: each length edit, each dimension, each field -- BITS and the DRI value among them
    for kind, variants in (("length", O.LENGTHS), ("dimension", O.DIMENSIONS), ("field", O.FIELDS)):
        assert {x.sub for x in cases if x.kind == kind} == set(variants), kind
    assert all(x.sub is None for x in cases if x.kind not in O.VARIANTS)
    src = O.damage_sources(prog)
    for x in cases:                                        # ... and the variant is true of the bytes
        base = src[x.base]
        if x.kind == "length":
            (m, a, e), = [g for g in O.segments(base) if x.data[g[1] + 2:g[1] + 4] != base[g[1] + 2:g[1] + 4]]
            new, old = int.from_bytes(x.data[a + 2:a + 4], "big"), e - a - 2
            assert x.data[:a + 2] + x.data[a + 4:] == base[:a + 2] + base[a + 4:], x.name
            assert new == {"0": 0, "1": 1, "65535": 65535}.get(x.sub, old + int(x.sub) if x.sub[0] in "+-" else None) or new == int(x.sub) - 1, x.name
        if x.kind == "field":
            at = [i for i in range(len(base)) if base[i] != x.data[i]]
            fields = O._fields(base, O.segments(base))
            assert len(x.data) == len(base) and all(any(f[0] == i and f[2] == x.sub for f in fields) for i in at), x.name
            # one field; or two neighbouring BITS counts, a code moved from one to the next
            assert len(at) == 1 or (x.sub == "BITS" and at[1] == at[0] + 1 and (x.data[at[0]], x.data[at[1]]) == (base[at[0]] - 1, base[at[1]] + 1)), x.name
        if x.kind == "dimension":
            (m, a, e), = [g for g in O.segments(base) if g[0] in (0xC0, 0xC1, 0xC2)]
            at = a + 5 + 2 * x.sub.startswith("width")
            assert int.from_bytes(x.data[at:at + 2], "big") == int(x.sub.split()[1]) and x.data[:at] + x.data[at + 2:] == base[:at] + base[at + 2:], x.name
    # a BITS damage that the parse takes: the same symbols under another code shape, which decides the lookup's contents
    assert any(x.sub == "BITS" and O.header_verdict(x.name, 256, prog).what == "parsed" for x in cases)
    # table slots above 3 in the scan header, the first one past the tables among them
    slots = [x.data[i] >> 4 if x.sub == "Td" else x.data[i] & 15 for x in cases if x.sub in ("Td", "Ta")
             for i in range(len(x.data)) if x.data[i] != src[x.base][i]]
    assert sum(v > 3 for v in slots) >= (1 if prog else 3) and (prog or 4 in slots), slots
    assert min(total) >= (8 if prog else 12), total
    for x in cases:
        a, b = (O.header_verdict(x.name, S, prog) for S in O.SUBSEQ)
        assert (a.what, a.pos) == (b.what, b.pos) and (a.inner is None or (a.inner.what, a.inner.bit) == (b.inner.what, b.inner.bit)), x.name
        # the damage lies in the marker segments: the entropy-coded bytes of the base are all there, in order, unless the file is cut
        base = src[x.base]
        if not x.kind.startswith("cut"):
            for a, e in O.M.scan_ranges(base, prog):
                assert base[a:e] in x.data, x.name
        assert x.data != base, x.name


@pytest.mark.parametrize("prog", TM.DECODERS)
def test_parse_entries_give_the_restatements_class_and_position(product_lib, prog):
    """v1c_jpeg_decode_info, v1c_jpeg_transcode_check and v1c_jpeg_compose_check (a whole-image output) on the sequential list,
    v1c_jpeg_prog_info on the progressive one: the code and the byte the parse stopped at, for every file.  None of them needs a device."""
    from vr180_convert_amd import _abi

    lib = product_lib
    lib.v1c_jpeg_decode_info.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    src = O.damage_sources(prog)
    bad = {}
    for x in O.header_damage(prog):
        v = O.header_verdict(x.name, 256, prog)
        code = ABI_CODE[v.what]
        if prog:
            info = _abi.JpegProgInfo()
            rc = lib.v1c_jpeg_prog_info(x.data, len(x.data), C.byref(info))
            got = [(rc, info.error_pos if rc else None)]
            if rc == 0:
                s = P.parse(x.data)
                assert (info.height, info.width, info.components, info.h_samp, info.v_samp, info.scans) == (s.h, s.w, s.nc, s.hs, s.vs, len(s.scans))
        else:
            info = TD._Info()
            rc = lib.v1c_jpeg_decode_info(x.data, len(x.data), C.byref(info))
            msg = lib.v1c_last_error().decode()
            got = [(rc, int(msg.split("(byte ")[1].split(")")[0]) if rc else None)]
            if rc == 0:
                s = D.parse(x.data)
                assert [getattr(info, f) for f, _ in TD._Info._fields_] == [s.h, s.w, s.nc, s.hs, s.vs, s.restart], x.name
            shape = O.shape_of(x.data, src[x.base])
            out = X.crop_output(shape)
            outs, keep = TX._xc_outputs([out], shape)
            pos = C.c_uint64(0)
            rc = lib.v1c_jpeg_transcode_check(x.data, len(x.data), 1, outs, C.byref(pos))
            got.append((rc, pos.value if rc else None))
            srcs, outs, keep = TF._xf_call([x.data], TF._as_compose([out]))
            pos = (C.c_uint64 * 1)()
            rc = lib.v1c_jpeg_compose_check(1, srcs, 1, outs, pos)
            got.append((rc, pos[0] if rc else None))
        if got != [(code, v.pos)] * len(got):
            bad[x.name] = (got, code, v.pos, v.why)
    assert not bad, bad


@pytest.mark.parametrize("prog", TM.DECODERS)
def test_host_builds_equal_restatement_on_the_damage_lists(emul_seq, emul_prog, emul_xf, prog):
    """the parse's class on every file; a file the parse takes then gives jpgdmg_cases' verdict -- code, bit, scan, rounds, pixels -- at
    both subsequence sizes, and on the sequential list the lossless entries give the restatement's code and bytes.  Against Pillow:
    where both decode the pixels are equal; the files on which one decodes and the other does not are printed and counted."""
    lib, diff = (emul_prog, TM.prog_differences) if prog else (emul_seq, TM.seq_differences)
    src = O.damage_sources(prog)
    bad, disagree = {}, []
    for x in O.header_damage(prog):
        for S in O.SUBSEQ:
            v = O.header_verdict(x.name, S, prog)
            rc, _ = (TP if prog else TD)._emul_info(lib, x.data)
            if rc != HOST_CODE[v.what]:
                bad[(x.name, S)] = f"parse rc {rc} for {v.what}"
            elif v.inner is not None and (d := diff(lib, x.data, S, v.inner)):
                bad[(x.name, S)] = d
            if prog:
                continue
            what = v.inner.what if v.inner else v.what
            out, code, want = O.transcode_want(x.data, what, src[x.base])
            rc, made = TX.run_emul(emul_xf, x.data, [out], S, O.shape_of(x.data, src[x.base]))
            if rc != code or (code == 0 and made[0][1] != want):
                bad[(x.name, S, "transcode")] = (rc, code)
            f = O.flip_want(x.data, what, src[x.base])
            if f is not None:
                out, code, want = f
                rc, made, _ = TF.run_emul(emul_xf, [x.data], [out], S)
                if rc != code or (code == 0 and made[0][1] != want):
                    bad[(x.name, S, "flip_h")] = (rc, code)
        v = O.header_verdict(x.name, 256, prog)
        ours = v.why if v.inner is None else None if v.inner.what == "decoded" else f"refused at bit {v.inner.bit}"
        try:
            got, theirs = _pillow(x.data), None
        except Exception as e:  # noqa: BLE001 (whatever Pillow raises is its reason)
            got, theirs = None, f"{type(e).__name__}: {e}"
        if (ours is None) != (theirs is None):
            disagree.append(f"{x.name}: Pillow: {theirs or 'decodes'}; restatement: {ours or 'decodes'}")
            if ours is None:                               # (decoded here, refused by libjpeg: a grey frame's factor outside 1 ... 4)
                assert x.sub in ("Hi", "Vi") and "gray" in x.base and x.how.endswith(("A", "E")), (x.name, x.how)
        elif ours is None:
            assert np.array_equal(got, v.inner.pixels), x.name
    print("\n".join(disagree))
    assert not bad, bad
    assert len(disagree) == PILLOW_DISAGREES[prog]


def test_python_layer_asks_the_progressive_parse_for_every_damaged_progressive_file():
    """``decode_jpeg_tensor(progressive=True)`` asks the sequential parse first and the progressive one where that refuses a file whose
    frame header is SOF2: on every file of the progressive damage list that route ends at the progressive restatement's class and byte,
    which is what tests/test_gpu_jpegodd.py then expects of the layer"""
    from vr180_convert_amd import jpeg_decode_device as J

    for x in O.header_damage(True):
        v = O.header_verdict(x.name, 256, True)
        with pytest.raises((D.Corrupt, D.Unsupported)) as e:
            D.parse(x.data)
        if e.type is D.Unsupported and J._is_progressive(x.data):
            continue
        assert (v.what, v.pos) == ("corrupt" if e.type is D.Corrupt else "unsupported", e.value.pos), x.name


# ---- the sanitizers -------------------------------------------------------------------------------------------------------------------
def _sanitized(tmp_path, harness, flag, name):
    exe = tmp_path / name
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fno-fast-math", flag, "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(harness)], check=True,
                   capture_output=True, timeout=600)
    return exe


def _clean(r):
    return r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


@pytest.mark.parametrize("prog", TM.DECODERS)
def test_standalone_sanitizer_run_of_the_decoders(tmp_path, prog):
    """both lists through the decoder's host build as a program of its own under the address and undefined-behaviour sanitizers, from
    heap copies of the files' exact sizes: no report, and the restatement's class for every file.  The GPU half sends these files."""
    exe = _sanitized(tmp_path, TP.HARNESS if prog else TD.HARNESS, "-DJPROG_MAIN" if prog else "-DJDEC_MAIN", "dec_san")
    files = {}
    for k, x in enumerate(PROG if prog else SEQ):
        p = tmp_path / f"legal_{k}.jpg"
        p.write_bytes(x.data)
        files[str(p)] = TM.CODE[O.legal_verdict(x.name, 256).what]
    for k, x in enumerate(O.header_damage(prog)):
        p = tmp_path / f"damage_{k}.jpg"
        p.write_bytes(x.data)
        v = O.header_verdict(x.name, 256, prog)
        files[str(p)] = HOST_CODE[v.what] if v.inner is None else TM.CODE[v.inner.what]
    r = subprocess.run([str(exe), *files], capture_output=True, text=True, timeout=600)
    assert _clean(r), r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 * len(files)
    for line in lines:
        assert int(line.split("rc=")[1].split()[0]) == files[line.split(" S=")[0]], line


def test_standalone_sanitizer_run_of_the_lossless_entries(tmp_path):
    """the sequential files of both lists through the composer's host build (which has the transcoder's) under the sanitizers: the
    whole image as it is (code 0: the transcoder's work) and mirrored"""
    exe = _sanitized(tmp_path, TF.HARNESS, "-DJXF_MAIN", "xf_san")
    lines, k = [], 0
    src = O.damage_sources(False)
    todo = [(x.data, O.legal_verdict(x.name, 256).what, None) for x in SEQ]
    for x in O.header_damage(False):
        v = O.header_verdict(x.name, 256, False)
        todo.append((x.data, v.inner.what if v.inner else v.what, src[x.base]))
    for data, what, fallback in todo:
        p = tmp_path / f"case_{k}.jpg"
        k += 1
        p.write_bytes(data)
        out, code, _ = O.transcode_want(data, what, fallback)
        wants = [(TF._as_compose([out])[0], code)]
        f = O.flip_want(data, what, fallback)
        if f is not None:
            wants.append((f[0], f[1]))
        for out, code in wants:
            lines.append(" ".join(str(v) for v in [code, 1, p, 1] + TF.spec_words([out], O.shape_of(data, fallback))))
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(manifest)], capture_output=True, text=True, timeout=900)
    assert _clean(r), (r.stdout[-2000:], r.stderr[-3000:])
    assert len(r.stdout.strip().splitlines()) == 2 * len(lines)
