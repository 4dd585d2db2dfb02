"""The lossless JPEG transcoder without a GPU: the restatement (jpgxc_ref.py) against an independent decoder -- the coefficients of
every output are the source's, and Pillow's pixels of grey and 4:4:4 outputs are Pillow's pixels of the source --; the product's host
code (jpegxc_core.hpp, jpegxc_host.hpp, behind the decoder's and in front of the encoder's) against the restatement, byte for byte;
what is refused, by the harness, by the library's host-only entries and by the Python layer, none of which touches a device; the
stand-alone sanitizer run; the resource notes of kernels_jpegxc.o."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jpg_cases as PC
import jpg_opt_ref as O
import jpg_ref as R
import jpgdec_cases as JC
import jpgdec_ref as D
import jpgdmg_cases as M
import jpgxc_cases as K
import jpgxc_ref as X

ROOT = Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "host_jpegxc" / "jpegxc_emul.hip"
CASES = K.cases()
CODES = {X.Unsupported: -2, X.Invalid: -1}


def spec_words(outputs, src=None):
    """the outputs as the harness and the sanitizer program take them"""
    words = []
    for o in outputs:
        r = o.get("restart_mcus")
        if r is None:
            mw = src.mw if src is not None else 8
            r = min(65535, -(-o["width"] // mw))
        words += [o["width"], o["height"], r, int(bool(o.get("optimize"))), len(o["regions"])]
        for reg in o["regions"]:
            words += list(reg)
    return words


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_jpegxc") / "libjpegxc_emul.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-fno-fast-math", "-o", str(out),
                    str(HARNESS)], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(out))
    lib.jxc_emul_transcode.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.jxc_emul_source_blocks.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    return lib


def run_emul(lib, data, outputs, S=0, src=None):
    """(return code, [(header, file), ...]) of the host build"""
    words = np.array(spec_words(outputs, src), np.int32)
    files = np.zeros(1 << 21, np.uint8)
    sizes = np.zeros(2 * max(len(outputs), 1), np.uint64)
    rc = lib.jxc_emul_transcode(data, len(data), S, words.ctypes.data, len(words), len(outputs), files.ctypes.data, files.size, sizes.ctypes.data)
    out, at = [], 0
    if rc == 0:
        for i in range(len(outputs)):
            head, total = int(sizes[2 * i]), int(sizes[2 * i + 1])
            out.append((files[at:at + head].tobytes(), files[at:at + total].tobytes()))
            at += total
    return rc, out


def _coefficients(data):
    """(info, (nblocks, 64) coefficients with the DC a value) of a file, by the decoder's restatement"""
    d = D.decode(data, check=False)
    return d.info, D.dc_values(d.info, d.coef)


# ---- the restatement against an independent decoder ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_outputs_hold_exactly_the_source_s_coefficients(name):
    """jpgdec_ref's decode of every output gives the source's coefficients of the gathered MCUs, the quantisation tables and the sampling
    factors of the source, and the size that was asked for"""
    data, outputs = CASES[name]
    s, coef = _coefficients(data)
    mcus = coef.reshape(s.mcuy, s.mcux, s.bpm, 64)
    for out, made in zip(outputs, K.reference(name)):
        t, got = _coefficients(made)
        assert (t.h, t.w, t.nc, t.hs, t.vs) == (out["height"], out["width"], s.nc, s.hs, s.vs)
        assert all(np.array_equal(t.q[t.tq[c]], s.q[s.tq[c]]) for c in range(s.nc))
        got = got.reshape(t.mcuy, t.mcux, t.bpm, 64)
        for sx, sy, nx, ny, dx, dy in out["regions"]:
            assert np.array_equal(got[dy:dy + ny, dx:dx + nx], mcus[sy:sy + ny, sx:sx + nx]), (name, (sx, sy))
        want = out.get("restart_mcus")
        assert t.restart == (t.mcux if want is None else want)


@pytest.mark.parametrize("name", [n for n in CASES if D.parse(CASES[n][0]).hs == 1])
def test_pillow_s_pixels_of_grey_and_444_outputs_are_the_source_s(name):
    """sample for sample, no tolerance: without chroma upsampling a pixel depends on its own block only.  (A subsampled output is held
    to its coefficients alone: libjpeg's chroma filter reads across the cut, so pixels next to it legitimately differ.)"""
    data, outputs = CASES[name]
    s = D.parse(data)
    whole = R.decode(data)
    for out, made in zip(outputs, K.reference(name)):
        got = R.decode(made)
        assert got.shape[:2] == (out["height"], out["width"])
        for sx, sy, nx, ny, dx, dy in out["regions"]:
            want = whole[8 * sy:8 * (sy + ny), 8 * sx:8 * (sx + nx)]
            part = got[8 * dy:8 * (dy + ny), 8 * dx:8 * (dx + nx)]
            hh, ww = min(want.shape[0], part.shape[0]), min(want.shape[1], part.shape[1])
            assert hh > 0 and ww > 0 and np.array_equal(part[:hh, :ww], want[:hh, :ww]), name


def test_case_list_sits_on_the_boundaries_it_is_for():
    blocks = {sum(len(X.gather(X.Source(d), o, X.check(X.Source(d), o))) for o in outs[:1]) for n, (d, outs) in CASES.items() if n.startswith("blocks_")}
    assert {31, 32, 33, 255, 256, 257, 258, 511, 512, 513, 516} <= blocks
    for kind in K.KINDS:
        s = D.parse(CASES[f"plus1_partial_column_{kind}"][0])
        m, n = K.KINDS[kind][2:]
        assert (s.w % m, s.h % n) == (1, 1) and CASES[f"plus1_partial_column_{kind}"][1][0]["width"] == 1
        s = D.parse(CASES[f"minus1_last_two_columns_{kind}"][0])
        assert (s.w % m, s.h % n) == (m - 1, n - 1)
        assert all(o["regions"][0][2] == 1 for o in CASES[f"split_2x1_{kind}"][1]) and len(CASES[f"swap_2x2_{kind}"][1][0]["regions"]) == 2
        for r in (1, 2, 7):
            d, outs = CASES[f"source_dri{r}_{kind}"]
            s = D.parse(d)
            sx, sy, nx, ny, _, _ = outs[0]["regions"][0]
            assert s.restart == r and (r == 1 or any(((sy + j) * s.mcux + sx) % r for j in range(ny)))  # a row starts inside an interval
        # a flat image: one symbol per table
        specs = O.dht_of(K.reference(f"optimize_flat_{kind}")[0])
        assert all(sum(bits) == 1 for _, bits, _ in specs)
    assert {o.get("restart_mcus") for _, outs in CASES.values() for o in outs} >= {None, 0, 1}
    assert D.decode(CASES[K.SLOW_ROUNDS][0], check=False).rounds > 5
    assert D.parse(CASES["dqt16_sof1"][0]).q[0].max() <= 255 and b"\xff\xc1" not in K.reference("dqt16_sof1")[0][:200]
    assert b"\xff\xc1" in K.reference("dqt16_wide")[0][:400] and D.parse(K.reference("dqt16_wide")[0]).q[0].max() == 300
    assert any(len(o["regions"]) >= 3 for _, outs in CASES.values() for o in outs)


def test_swapping_twice_gives_the_file_s_coefficients_back():
    for name in ("swap_2x2_gray", "swap_2x2_444", "swap_2x2_420", "noise_q100_444_swap", "swap_dri7_420"):
        data = CASES[name][0]
        s, coef = _coefficients(data)
        once = X.swap_sbs_jpeg(data)
        t, back = _coefficients(X.swap_sbs_jpeg(once))
        assert (t.h, t.w) == (s.h, s.w) and np.array_equal(back, coef), name
        assert not np.array_equal(_coefficients(once)[1], coef)


@pytest.mark.parametrize("cn,sub,restart", [(3, "420", None), (3, "444", 3), (1, "420", 1), (3, "420", 65535)])
def test_split_of_an_encoded_file_is_the_encoder_s_file_of_each_half(cn, sub, restart):
    """a side-by-side file by the encoder's restatement, split with its restart interval: every half is, byte for byte, what the
    encoder's restatement writes for the half's coefficients -- its header with the quality's tables and its scan"""
    quality, h, w = 85, 40, 96
    img = PC.smooth(h, w, cn, 900 + cn)
    data = R.encode(img, quality, sub, restart)
    zz = R.coefficients(img, quality, sub)
    g = R.Geom(h, w, cn, sub, restart)
    mcus = zz.reshape(g.mcuy, g.mcux, g.bpm, 64)
    half = X.split_sbs_jpeg(data, restart_mcus=restart)
    for side, made in enumerate(half):
        gh = R.Geom(h, w // 2, cn, sub, restart)
        own = np.ascontiguousarray(mcus[:, side * gh.mcux:(side + 1) * gh.mcux]).reshape(-1, 64)
        assert made == R.headers(gh, quality) + R.scan(own, gh) + b"\xff\xd9"


def test_whole_image_transcode_of_an_encoded_file_is_the_file():
    img = PC.smooth(33, 47, 3, 910)
    for sub in ("420", "444"):
        data = R.encode(img, 90, sub, 2)
        assert X.transcode_jpeg(data, restart_mcus=2) == data
        assert X.transcode_jpeg(data, restart_mcus=2, optimize=True) == O.encode(img, 90, sub, 2)


# ---- the product's host code against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_host_build_equals_restatement(emul, name):
    """header and scan, byte for byte, at two subsequence sizes: standard and optimised tables, with and without restart intervals"""
    data, outputs = CASES[name]
    src = X.Source(data)
    for S in (256, 0):
        rc, made = run_emul(emul, data, outputs, S, src)
        assert rc == 0, (name, rc)
        for (head, whole), out, want in zip(made, outputs, K.reference(name)):
            _, want_head, want_scan = X.parts(src, out)
            assert head == want_head, name
            assert whole == want == want_head + want_scan + b"\xff\xd9", name


def test_source_blocks_of_the_host_build(emul):
    """jpegxc_core.hpp's block map against the restatement's gather over MCU indices, uncovered MCUs included"""
    rng = np.random.default_rng(3)
    for bpm in (1, 3, 6):
        for _ in range(20):
            smx, smy = int(rng.integers(1, 9)), int(rng.integers(1, 7))
            nx, ny = int(rng.integers(1, smx + 1)), int(rng.integers(1, smy + 1))
            sx, sy = int(rng.integers(0, smx - nx + 1)), int(rng.integers(0, smy - ny + 1))
            dx, dy = int(rng.integers(0, 3)), int(rng.integers(0, 3))
            dmx, dmy = dx + nx + int(rng.integers(0, 2)), dy + ny + int(rng.integers(0, 2))
            want = np.full((dmy, dmx, bpm), 0xFFFFFFFF, np.int64)
            src = (np.arange(smx * smy).reshape(smy, smx)[:, :, None] * bpm + np.arange(bpm)[None, None, :])
            want[dy:dy + ny, dx:dx + nx] = src[sy:sy + ny, sx:sx + nx]
            got = np.zeros(dmx * dmy * bpm, np.uint32)
            reg = np.array([sx, sy, nx, ny, dx, dy], np.int32)
            emul.jxc_emul_source_blocks(reg.ctypes.data, 1, smx, dmx, dmy, bpm, got.ctypes.data)
            assert np.array_equal(got.astype(np.int64), want.reshape(-1))


# ---- what is refused -------------------------------------------------------------------------------------------------------------------
def test_refusals_by_the_restatement_and_the_host_build(emul):
    for name, (data, outputs, exc) in K.refused().items():
        with pytest.raises(exc):
            X.transcode(data, outputs)
        rc, _ = run_emul(emul, data, outputs)
        assert rc == CODES[exc], (name, rc)
    for name, (data, outputs, by_parse) in K.corrupt().items():
        rc, _ = run_emul(emul, data, outputs)
        assert rc == -5, (name, rc)
    # valid syntax, numbers beyond 8-bit samples: coefficients the encoder's tables do not code
    for name, (data, outputs) in K.out_of_range().items():
        with pytest.raises(X.Unsupported):
            X.transcode(data, outputs)
        rc, _ = run_emul(emul, data, outputs)
        assert rc == -2, (name, rc)
    for name, (data, outputs) in K.excluded_blocks().items():  # the same kind of block, left out by the cut: taken
        rc, made = run_emul(emul, data, outputs, src=X.Source(data))
        assert rc == 0 and [m[1] for m in made] == X.transcode(data, outputs), (name, rc)
    for name, data in JC.extreme_cases().items():  # (16-bit quantiser entries, coefficients inside the range: taken)
        s = D.parse(data)
        rc, made = run_emul(emul, data, [dict(width=s.w, height=s.h, regions=[(0, 0, s.mcux, s.mcuy, 0, 0)])], src=X.Source(data))
        assert rc == 0 and made[0][1] == X.transcode_jpeg(data), (name, rc)


def _xc_outputs(outputs, src=None):
    from vr180_convert_amd.jpeg_transcode_device import XcOutput, XcRegion

    outs = (XcOutput * len(outputs))()
    keep = []
    for o, spec in zip(outs, outputs):
        arr = (XcRegion * max(len(spec["regions"]), 1))(*[XcRegion(*r) for r in spec["regions"]])
        keep.append(arr)
        r = spec.get("restart_mcus")
        o.width, o.height = spec["width"], spec["height"]
        o.restart_mcus = min(65535, -(-spec["width"] // (src.mw if src else 8))) if r is None else r
        o.optimize, o.nregions, o.regions = int(bool(spec.get("optimize"))), len(spec["regions"]), arr
    return outs, keep


def test_library_refuses_without_a_device(product_lib):
    """the host-only entries of the C ABI: the check, the bound and the header; and v1c_jpeg_transcode itself, whose checks all come
    before its first device call (device -1 would be its next complaint)"""
    from vr180_convert_amd import _native

    lib = _native.lib()
    for name, (data, outputs, exc) in K.refused().items():
        outs, keep = _xc_outputs(outputs)
        assert lib.v1c_jpeg_transcode_check(data, len(data), len(outputs), outs, None) == CODES[exc], name
        buf = np.zeros(1 << 20, np.uint8)
        for o in outs:
            o.out_host, o.capacity = buf.ctypes.data, buf.size
        assert lib.v1c_jpeg_transcode(-1, None, data, len(data), len(outputs), outs, 0, None) == CODES[exc], name
    for name, (data, outputs, by_parse) in K.corrupt().items():
        outs, keep = _xc_outputs(outputs)
        assert lib.v1c_jpeg_transcode_check(data, len(data), len(outputs), outs, None) == (-5 if by_parse else 0), name
    for name, (data, outputs) in CASES.items():
        src = X.Source(data)
        outs, keep = _xc_outputs(outputs, src)
        assert lib.v1c_jpeg_transcode_check(data, len(data), len(outputs), outs, None) == 0, name
        # with every check passed the next complaint is the device's: nothing before it touched one
        buf = np.zeros(1, np.uint8)
        for o in outs:
            o.out_host, o.capacity = buf.ctypes.data, 1 << 40
        assert lib.v1c_jpeg_transcode(-1, None, data, len(data), len(outputs), outs, 0, None) == -4, name
        for o in outs:
            o.capacity = 16
        assert lib.v1c_jpeg_transcode(-1, None, data, len(data), len(outputs), outs, 0, None) == -1 and b"capacity" in lib.v1c_last_error()
    data, outputs = CASES["whole_2x2_420"]
    outs, keep = _xc_outputs(outputs, X.Source(data))
    assert lib.v1c_jpeg_transcode_check(None, 0, 1, outs, None) == -1 and lib.v1c_jpeg_transcode_check(data, len(data), 0, outs, None) == -1
    assert lib.v1c_jpeg_transcode_check(data, len(data), 17, outs, None) == -1 and lib.v1c_jpeg_transcode_check(data, len(data), 1, None, None) == -1
    assert lib.v1c_jpeg_transcode(0, None, data, len(data), 1, outs, 100, None) == -1 and b"subseq_bits" in lib.v1c_last_error()


def test_library_header_and_bound_equal_the_restatement(product_lib):
    from vr180_convert_amd import _native

    lib = _native.lib()
    for name, (data, outputs) in CASES.items():
        src = X.Source(data)
        for out in outputs:
            g = X.check(src, out)
            _, want_head, _ = X.parts(src, out)
            specs = O.tables(X.gather(src, out, g), g) if out.get("optimize") else None
            dht = O.dht_body(specs) if specs else None
            head = (C.c_uint8 * 2048)()
            n = lib.v1c_jpeg_header_xc(data, len(data), out["width"], out["height"], g.dri, dht, len(dht) if dht else 0, head, 2048)
            assert n > 0 and bytes(head[:n]) == want_head, name
            bound = lib.v1c_jpeg_transcode_bound(data, len(data), out["width"], out["height"], g.dri)
            assert bound == 2 * (g.nblocks * ((R.MAX_BLOCK_BITS + 7) // 8) + g.nint) + 2 * g.nint  # (jpg_ref.bound's rule for this geometry)
            assert bound >= len(X.parts(src, out)[2])
    data = CASES["whole_2x2_420"][0]
    head = (C.c_uint8 * 2048)()
    assert lib.v1c_jpeg_header_xc(data, len(data), 32, 32, 2, b"\x00" * 20, 20, head, 2048) == -1 and b"dht" in lib.v1c_last_error()
    assert lib.v1c_jpeg_header_xc(data, len(data), 32, 32, 2, None, 0, head, 100) == -1 and lib.v1c_jpeg_header_xc(data, len(data), 0, 32, 2, None, 0, head, 2048) == -1
    assert lib.v1c_jpeg_header_xc(K.refused()["progressive"][0], len(K.refused()["progressive"][0]), 32, 32, 2, None, 0, head, 2048) == -2
    assert lib.v1c_jpeg_transcode_bound(K.refused()["sampling_411"][0], len(K.refused()["sampling_411"][0]), 32, 32, 2) == 0


def test_python_layer_refuses_before_any_device_call(monkeypatch):
    """NotImplementedError for a file outside scope, CorruptJPEG for a damaged one, ValueError for geometry; the device is never asked for"""
    import vr180_convert_amd as V
    from vr180_convert_amd import jpeg_transcode_device as T, remapper
    from vr180_convert_amd.jpeg_decode_device import CorruptJPEG

    def no_device(*a, **k):
        raise AssertionError("a refused call asked for the device")

    monkeypatch.setattr(remapper, "_device", no_device)
    assert V.transcode_jpeg is T.transcode_jpeg and V.split_sbs_jpeg is T.split_sbs_jpeg and V.swap_sbs_jpeg is T.swap_sbs_jpeg
    ref = K.refused()
    for name in ("progressive", "sampling_411", "three_table_classes"):
        for call in (T.transcode_jpeg, T.split_sbs_jpeg, T.swap_sbs_jpeg):
            with pytest.raises(NotImplementedError):
                call(ref[name][0])
    with pytest.raises(NotImplementedError, match="overlap"):
        T.transcode_regions(ref["overlapping_regions"][0], ref["overlapping_regions"][1])
    for name in ("uncovered_mcus", "region_outside_source", "region_outside_output", "size_below_the_regions", "no_regions", "seventeen_regions",
                 "restart_too_large"):
        with pytest.raises(ValueError):
            T.transcode_regions(ref[name][0], ref[name][1])
    for name, (data, outputs, by_parse) in K.corrupt().items():
        if by_parse:
            with pytest.raises(CorruptJPEG):
                T.transcode_jpeg(data)
    base = JC.pillow(PC.smooth(48, 80, 3, 920), 90, "420")          # 5 x 3 MCUs of 16 x 16: half the width is no multiple of 16
    for crop in ((8, 0, 16, 16), (0, 8, 16, 16), (16, 16, 80, 16), (0, 0, 0, 16), (-16, 0, 16, 16)):
        with pytest.raises(ValueError):
            T.transcode_jpeg(base, crop=crop)
    for call in (T.split_sbs_jpeg, T.swap_sbs_jpeg):
        with pytest.raises(ValueError, match="half"):
            call(base)
        with pytest.raises(ValueError, match="half"):
            call(JC.pillow(PC.smooth(16, 33, 1, 921), 90))            # an odd width
    with pytest.raises(ValueError, match="restart_mcus"):
        T.transcode_jpeg(base, restart_mcus=70000)
    # the same geometry rules as the restatement's
    src = X.Source(base)
    h, w, mw, mh = T.probe_mcu(base)
    assert (h, w, mw, mh) == (48, 80, 16, 16)
    got = T._crop_output(h, w, mw, mh, (16, 32, 50, 9), {})
    assert got == X.crop_output(src, (16, 32, 50, 9))


# ---- the stand-alone sanitizer run -----------------------------------------------------------------------------------------------------
def test_standalone_sanitizer_run(tmp_path):
    """the host build as a program of its own under the address and undefined-behaviour sanitizers: every supported case, the refused
    and the corrupt ones, one file truncated at every length and every damaged scan of tests/jpgdmg_cases.py, from heap copies of exact
    sizes; any report fails the run"""
    exe = tmp_path / "jpegxc_san"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fno-fast-math", "-DJXC_MAIN", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(HARNESS)], check=True,
                   capture_output=True, timeout=600)
    lines, k = [], 0

    def add(data, outputs, want, src=None):
        nonlocal k
        p = tmp_path / f"case_{k}.jpg"
        k += 1
        p.write_bytes(data)
        lines.append(" ".join(str(v) for v in [p, want, len(outputs)] + spec_words(outputs, src)))

    for name, (data, outputs) in CASES.items():
        add(data, outputs, 0, X.Source(data))
    for name, (data, outputs, exc) in K.refused().items():
        add(data, outputs, CODES[exc])
    for name, (data, outputs, by_parse) in K.corrupt().items():
        add(data, outputs, -5)
    data, outputs = CASES["source_dri2_420"]
    cuts = list(range(0, 700, 7)) + list(range(700, len(data), 41))
    for n in cuts:
        add(data[:n], outputs, -5, X.Source(data))
    # the damaged scans of tests/jpgdmg_cases.py, which do reach the entropy decoder, as the source of a whole-image transcode
    for x in M.sequential_cases():
        out, code, _ = M.transcode_want(x.name)
        add(x.data, [out], code, M.shape_of(x))
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(manifest)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-3000:])
    assert len(r.stdout.strip().splitlines()) == 2 * len(lines)


# ---- the code object ---------------------------------------------------------------------------------------------------------------------
def test_kernels_jpegxc_use_no_scratch_and_spill_nothing(tmp_path, product_lib):
    from test_resource_budget import kernel_metadata

    obj = ROOT / "vr180_convert_amd" / "csrc" / "kernels_jpegxc.o"
    assert obj.exists(), "kernels_jpegxc.o is built by __graft_entry__.build() / make"
    kernels = kernel_metadata(tmp_path, obj)
    assert sorted(k[".name"].split("k_jxc_")[1][:4] for k in kernels) == ["gath", "hist", "pack", "size"]
    bad = [(k[".name"], k[".private_segment_fixed_size"], k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for k in kernels
           if k[".private_segment_fixed_size"] or k[".sgpr_spill_count"] or k[".vgpr_spill_count"]]
    assert not bad, bad
    assert all(k[".wavefront_size"] == 64 for k in kernels)
    assert [k[".group_segment_fixed_size"] for k in kernels if "gather" in k[".name"]] == [0]  # the region list comes with the arguments
