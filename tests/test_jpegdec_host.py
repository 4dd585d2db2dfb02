"""The device JPEG decoder without a GPU: the restatement (jpgdec_ref.py) against itself, against a float64 inverse DCT and against
Pillow; the product's jpegdec_core.hpp / jpegdec_host.hpp run on the host, in a sequential copy of the kernels' decomposition, against
the restatement value for value; the same build under the address and undefined-behaviour sanitizers as a stand-alone program; the
case list the GPU half shares; the C ABI's argument checks; the resource budget of kernels_jpegdec.o; the device_decode plumbing."""
import ctypes as C
import io
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jpg_cases as PC
import jpg_ref as R
import jpgdec_cases as DC
import jpgdec_ref as D
import jpgdmg_cases as M

ROOT = Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "host_jpegdec" / "jpegdec_emul.hip"
DOCS_JPG = ROOT / "tests" / "golden" / "ref_docs" / "test.jpg"
CASES = DC.supported_cases()
EXTREME = DC.extreme_cases()
SUBSEQ = (256, 1024, 4096)

# The restatement against Pillow 12.2 (libjpeg-turbo 3.1), ``Image.open(...).convert("RGB")``: the largest absolute difference per
# sample and the share of differing samples, measured on every supported case and on tests/golden/ref_docs/test.jpg.  Both sides are
# deterministic CPU code, so the test asserts exactly these values; INTEGRATION.md section 8 quotes them.
PILLOW_MAX_DIFF = 0
PILLOW_SHARE_DIFFERING = 0.0


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_jpegdec") / "libjpegdec_emul.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-fno-fast-math", "-o", str(out),
                    str(HARNESS)], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(out))
    vp, u32 = C.c_void_p, C.c_uint32
    lib.jdec_emul_info.argtypes = [C.c_char_p, C.c_uint64, vp]
    lib.jdec_emul_decode.argtypes = [C.c_char_p, C.c_uint64, u32, C.c_int, vp, vp, vp, u32, vp, vp]
    return lib


def _pillow_bgr(data):
    from PIL import Image

    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])


def _emul_info(lib, data):
    info = np.zeros(8, np.int32)
    return lib.jdec_emul_info(data, len(data), info.ctypes.data), info


def _emul_decode(lib, data, S, cn=3):
    rc, info = _emul_info(lib, data)
    assert rc == 0
    h, w, nblocks = int(info[0]), int(info[1]), int(info[7])
    cap = len(data) * 8 // 256 + int(info[6]) + 1
    coef = np.zeros((nblocks, 64), np.int16)
    states, counts, report = np.zeros((cap, 3), np.uint32), np.zeros(cap, np.uint32), np.zeros(4, np.uint32)
    px = np.zeros((h, w, cn), np.uint8)
    rc = lib.jdec_emul_decode(data, len(data), S, cn, coef.ctypes.data, states.ctypes.data, counts.ctypes.data, cap, report.ctypes.data,
                              px.ctypes.data)
    n = int(report[1])
    return rc, coef, states[:n], counts[:n], report, px


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_iteration_equals_sequential_decoder(name):
    """for three subsequence sizes: the iteration's entry states are the plain decoder's wherever that one passes a subsequence's first
    bit, and the last pass gives its coefficients (D.decode asserts both); the pixels do not depend on the size"""
    ref = [DC.reference(name, S) for S in SUBSEQ]
    for r, S in zip(ref, SUBSEQ):
        coef, states = D.sequential(r.stream)
        assert np.array_equal(coef, r.coef)
        assert all(a is None or a == b for a, b in zip(states, r.entry)) and states[0] is not None
        assert r.rounds <= r.subsequences + 1 and r.subsequences == len(r.entry)
        assert np.array_equal(r.pixels, ref[0].pixels) and np.array_equal(r.coef, ref[0].coef)
    assert ref[0].subsequences >= ref[1].subsequences >= ref[2].subsequences


def test_restatement_reads_what_the_encoders_restatement_wrote():
    """the decoder's coefficients of a file by jpg_ref.encode are the encoder's"""
    for name, args in [("midrow_420_r3", (PC.smooth(40, 72, 3, 50), 95, "420")), ("dri1_444", (PC.smooth(40, 72, 3, 52), 95, "444")),
                       ("dri2_420_noise", (PC.noise(48, 64, 3, 62), 100, "420"))]:
        r = DC.reference(name, 256)
        assert np.array_equal(D.dc_values(r.info, r.coef), R.coefficients(*args))


@pytest.mark.parametrize("name", [n for n in CASES if n.endswith("gray") or n in ("only_63", "zero_runs", "swing_q100", "flat_gray_200")])
def test_grey_samples_are_within_one_of_the_float_idct(name):
    """independent of the product and of Pillow: the rounded float64 inverse DCT of the dequantised coefficients"""
    r = DC.reference(name)
    s = r.info
    assert s.nc == 1
    f = np.zeros((s.nblocks, 64))
    f[:, R.ZIGZAG] = D.dc_values(s, r.coef).astype(np.float64)
    f = (f * s.q[s.tq[0]]).reshape(-1, 8, 8)
    c = PC._basis()
    want = np.clip(np.rint(np.einsum("ux,nuv,vy->nxy", c, f, c) + 128), 0, 255)
    assert np.abs(D.samples(s, D.dc_values(s, r.coef)).astype(np.float64) - want).max() <= 1


def test_restatement_against_pillow():
    worst, differing, total = 0, 0, 0
    for name, data in CASES.items():
        d = np.abs(DC.reference(name).pixels.astype(np.int64) - _pillow_bgr(data))
        worst, differing, total = max(worst, int(d.max())), differing + int((d > 0).sum()), total + d.size
    data = DOCS_JPG.read_bytes()
    d = np.abs(D.decode(data, 4096, check=False).pixels.astype(np.int64) - _pillow_bgr(data))
    print(f"cases: max {worst}, differing {differing} of {total}; docs image: max {int(d.max())}, differing {int((d > 0).sum())} of {d.size}")
    worst, differing, total = max(worst, int(d.max())), differing + int((d > 0).sum()), total + d.size
    assert worst == PILLOW_MAX_DIFF and differing / total == PILLOW_SHARE_DIFFERING


# ---- the case list ------------------------------------------------------------------------------------------------------------------
def test_case_list_sits_on_the_boundaries_it_is_for():
    info = {n: D.parse(d) for n, d in CASES.items()}
    for h, w in PC.SIZES:
        for kind, hv in (("444", (1, 1)), ("422", (2, 1)), ("420", (2, 2)), ("gray", (1, 1))):
            s = info[f"size_{h}x{w}_{kind}"]
            assert (s.h, s.w, s.hs, s.vs, s.nc) == (h, w, *hv, 1 if kind == "gray" else 3) and s.restart == 0
    nodri = [n for n, s in info.items() if s.restart == 0]
    dri = {n: s for n, s in info.items() if s.restart}
    assert any(s.restart == 1 and s.nseg > 8 for s in dri.values())                              # DRI 1, RSTm wraps
    assert any(s.restart % s.mcux and s.nseg > 2 for s in dri.values())                          # ends mid-row
    assert any(s.restart == s.nmcu for s in dri.values()) and any(s.nmcu < s.restart < 65535 for s in dri.values())
    assert any(s.restart == 65535 for s in dri.values()) and max(s.nseg for s in dri.values()) == 45
    assert {(s.hs, s.vs) for s in dri.values()} == {(1, 1), (2, 1), (2, 2)}
    # states: a subsequence entered mid-block, one entered in a later block of its MCU, one entered off the grid
    entries = [(n, e, sub) for n in CASES for e, sub in zip(DC.reference(n, 256).entry, DC.reference(n, 256).stream.subs)]
    assert any(e[1] != 0 for _, e, _ in entries) and any(e[2] != 0 for _, e, _ in entries) and any(e[0] != sub[1] for _, e, sub in entries)
    assert any(e[0] == sub[1] and not first for n in CASES for e, sub, first in
               zip(DC.reference(n, 256).entry, DC.reference(n, 256).stream.subs, DC.reference(n, 256).stream.first))  # ... and on it
    # a 0xFF / 0x00 pair with the 0xFF at the end of a 16-byte piece, and one with it at the start
    def pair_offsets(n):
        s = info[n]
        scan = CASES[n][s.scan_start:s.scan_start + s.scan_len]
        return {i % 16 for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] == 0}
    offs = set().union(*(pair_offsets(n) for n in CASES if n.startswith("noise")))
    assert {15, 0, 14} <= offs, sorted(offs)
    # RSTm on either side of a piece boundary too
    s = info["dri1_444"]
    scan = CASES["dri1_444"][s.scan_start:s.scan_start + s.scan_len]
    assert len({i % 16 for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7}) >= 12
    assert any(DC.reference(n, 256).rounds >= 3 for n in nodri)
    assert any(DC.reference(n, 256).subsequences > 256 for n in nodri)                            # more than a workgroup's lanes
    assert DC.reference("noise_q100_444", 256).subsequences > 512
    # EOB-only blocks: well over a hundred blocks in one subsequence
    assert max(DC.reference("flat_420").counts) > 150 and not DC.reference("flat_420").coef[:, 1:].any()
    # blocks without EOB, ZRL runs, the largest categories, stuffed bytes
    assert DC.reference("only_63").coef[:, 63].all() and DC.reference("zero_runs").coef[3, 63] != 0
    zz = DC.reference("zero_runs").coef
    runs = set()
    for b in zz:
        nz = np.nonzero(b[1:])[0] + 1
        runs |= set((nz - np.concatenate([[0], nz[:-1]]) - 1).tolist())
    assert {15, 16, 17, 33} <= runs
    sw = DC.reference("swing_q100").coef
    assert int(np.abs(sw[:, 0]).max()).bit_length() == 11 and int(np.abs(sw[:, 1:]).max()).bit_length() == 10
    assert all(len(pair_offsets(n)) >= 8 for n in CASES if n.startswith("noise_q100"))
    # optimised tables differ from Annex K's, and a wrong entry state meets bits that start no code
    st = DC.reference("optimised_420", 256).stream
    assert info["optimised_420"].ac[0].bits != R.AC_LUMA[0]
    assert any(0 in (st.ac_lut[0][w], st.dc_lut[0][w]) for w in range(0, 65536, 16))
    assert {"quality_1", "quality_100", "dqt16_sof1", "com_app1", "fill_bytes", "fill_bytes_rst", "merged_dht", "junk_after_eoi"} <= set(CASES)
    assert max(int(info["dqt16_sof1"].q[0].max()), 0) == int(info["com_app1"].q[0].max()) and b"\xff\xc1" in CASES["dqt16_sof1"][:700]
    assert CASES["merged_dht"].count(b"\xff\xc4") == 1 and CASES["com_app1"].count(b"\xff\xc4") == 4
    for n in ("dqt16_sof1", "com_app1", "fill_bytes", "merged_dht", "junk_after_eoi", "adobe_ycc"):
        assert np.array_equal(DC.reference(n).pixels, DC.reference("com_app1").pixels)       # edits that leave the image alone
    assert np.array_equal(DC.reference("fill_bytes_rst").pixels, DC.reference("midrow_420_r3").pixels)


def test_extreme_files_meet_the_saturation():
    """16-bit quantiser entries times the coefficients of these files pass 16 bits, so the contract's saturation acts, and the
    restatement's own 64-bit arithmetic is what the product is held to"""
    for name, data in EXTREME.items():
        r = DC.reference(name)
        s = r.info
        q = np.stack([s.q[s.tq[c]] for c in s.comp])
        f = np.zeros((s.nblocks, 64), np.int64)
        f[:, R.ZIGZAG] = D.dc_values(s, r.coef).astype(np.int64)
        assert np.abs(f * np.tile(q, (s.nmcu, 1))).max() > 5 * 32768, name
        assert np.array_equal(DC.reference(name, 256).pixels, r.pixels)


def test_unsupported_and_corrupt_files_by_the_restatement():
    for name, data in DC.unsupported_cases().items():
        with pytest.raises(D.Unsupported):
            D.parse(data)
    for name, (data, by_parse) in DC.corrupt_cases().items():
        if by_parse:
            with pytest.raises(D.Corrupt):
                D.parse(data)
        else:
            D.parse(data)
            for S in (256, 1024):
                with pytest.raises(D.Corrupt):
                    D.decode(data, S, check=False)


# ---- the product's arithmetic on the host -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES) + list(EXTREME))
def test_product_host_code_equals_restatement(emul, name):
    """coefficients, entry states, block counts, segments, subsequences, rounds and pixels, through a sequential copy of the kernels'
    decomposition (drop counts per piece, scans, placement, two exit buffers with the skip rule, DC subtraction)"""
    for S in SUBSEQ:
        want = DC.reference(name, S)
        rc, coef, states, counts, report, px = _emul_decode(emul, {**CASES, **EXTREME}[name], S)
        assert rc == 0
        assert report[:3].tolist() == [want.segments, want.subsequences, want.rounds]
        assert np.array_equal(coef, want.coef)
        assert [tuple(s) for s in states.tolist()] == want.entry
        assert counts.tolist() == want.counts
        assert np.array_equal(px, want.pixels)
    if want.info.nc == 1 and name in CASES:
        rc, *_, px = _emul_decode(emul, CASES[name], 0, cn=1)
        assert rc == 0 and np.array_equal(px[..., 0], D.decode(CASES[name], 0, channels=1, check=False).pixels)


def test_info_of_the_host_parse(emul):
    for name, data in CASES.items():
        s = D.parse(data)
        rc, info = _emul_info(emul, data)
        assert rc == 0 and info.tolist() == [s.h, s.w, s.nc, s.hs, s.vs, s.restart, s.nseg, s.nblocks], name
    for name, data in DC.unsupported_cases().items():
        assert _emul_info(emul, data)[0] == 1, name
    for name, (data, by_parse) in DC.corrupt_cases().items():
        assert _emul_info(emul, data)[0] == (2 if by_parse else 0), name


def test_corrupt_files_on_the_host_build(emul):
    for name, (data, by_parse) in DC.corrupt_cases().items():
        for S in (256, 1024):
            info = np.zeros(8, np.int32)
            report = np.zeros(4, np.uint32)
            rc = emul.jdec_emul_decode(data, len(data), S, 3, None, None, None, 0, report.ctypes.data, None)
            assert rc == (2 if by_parse else 3), (name, rc)


def test_standalone_sanitizer_run(tmp_path):
    """the host build as a program of its own under the address and undefined-behaviour sanitizers: every case, the unsupported and
    the corrupt ones included, and every damaged scan of tests/jpgdmg_cases.py, from heap copies of the files' exact sizes; any report
    fails the run"""
    exe = tmp_path / "jpegdec_san"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fno-fast-math", "-DJDEC_MAIN", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(HARNESS)], check=True,
                   capture_output=True, timeout=600)
    files = {}
    for group, cases in (("ok", {**CASES, **EXTREME}), ("unsup", DC.unsupported_cases()), ("bad", {n: d for n, (d, _) in DC.corrupt_cases().items()})):
        for name, data in cases.items():
            p = tmp_path / f"{group}_{name}.jpg"
            p.write_bytes(data)
            files[str(p)] = group
    # truncations of one file at every length: headers cut anywhere, scans cut anywhere
    base = CASES["midrow_420_r3"]
    for n in list(range(0, 700, 7)) + list(range(700, len(base), 53)):
        p = tmp_path / f"cut_{n}.jpg"
        p.write_bytes(base[:n])
        files[str(p)] = "cut"
    # the damaged scans of tests/jpgdmg_cases.py, which do reach the entropy decoder: the exit code is the restatement's class
    for k, x in enumerate(M.sequential_cases()):
        p = tmp_path / f"dmg_{k}.jpg"
        p.write_bytes(x.data)
        files[str(p)] = M.verdict(x.name, 256, False).what
    r = subprocess.run([str(exe), *files], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 * len(files)
    for line in lines:
        path, rc = line.split(" S=")[0], int(line.split("rc=")[1].split()[0])
        want = {"ok": (0,), "unsup": (1,), "bad": (2, 3), "cut": (2, 3), "decoded": (0,), "unsupported": (1,), "parse": (2,),
                "refused": (3,)}[files[path]]
        assert rc in want, line


# ---- the library without a device ---------------------------------------------------------------------------------------------------
class _Info(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("height", "width", "components", "h_samp", "v_samp", "restart_interval")]


def test_decode_info_and_argument_checks_without_device(product_lib):
    lib = product_lib
    lib.v1c_jpeg_decode_info.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    info = _Info()
    for name, data in CASES.items():
        s = D.parse(data)
        assert lib.v1c_jpeg_decode_info(data, len(data), C.byref(info)) == 0, name
        assert [getattr(info, f) for f, _ in _Info._fields_] == [s.h, s.w, s.nc, s.hs, s.vs, s.restart]
    for name, data in DC.unsupported_cases().items():
        assert lib.v1c_jpeg_decode_info(data, len(data), C.byref(info)) == -2, name
    for name, (data, by_parse) in DC.corrupt_cases().items():
        assert lib.v1c_jpeg_decode_info(data, len(data), C.byref(info)) == (-5 if by_parse else 0), name
    assert b"byte" in lib.v1c_last_error()
    assert lib.v1c_jpeg_decode_info(None, 10, C.byref(info)) == -1 and lib.v1c_jpeg_decode_info(b"abcd", 4, None) == -1
    assert lib.v1c_jpeg_decode_info(b"", 0, C.byref(info)) == -5 and lib.v1c_jpeg_decode_info(b"\xff\xd8\xff", 3, C.byref(info)) == -5

    lib.v1c_jpeg_decode.argtypes = [C.c_int, C.c_void_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_int64, C.c_int, C.c_uint32, C.c_void_p]
    out = np.zeros(1 << 16, np.uint8)  # stands in for the device pointer: validation fails before any device call
    data = CASES["size_17x17_420"]

    def call(file=data, size=len(data), dst=out.ctypes.data, pitch=17 * 3, cn=3, S=0):
        return lib.v1c_jpeg_decode(0, None, file, size, dst, pitch, cn, S, None)

    def err():
        return lib.v1c_last_error().decode()

    assert call(file=None) == -1 and "NULL" in err() and call(dst=None) == -1
    assert call(cn=2) == -1 and "out_cn" in err() and call(cn=4) == -1
    assert call(cn=1) == -1 and "one component" in err()
    assert call(S=128) == -1 and "subseq_bits" in err() and call(S=300) == -1 and call(S=1 << 25) == -1
    assert call(pitch=50) == -1 and "pitch" in err()
    for name, d in DC.unsupported_cases().items():
        assert call(file=d, size=len(d)) == -2, name
    for name, (d, by_parse) in DC.corrupt_cases().items():
        if by_parse:
            assert call(file=d, size=len(d)) == -5, name
    assert call(size=len(data) - 2) == -5 and "EOI" in err()


def test_kernels_jpegdec_use_no_scratch_and_spill_nothing(tmp_path, product_lib):
    from test_resource_budget import kernel_metadata

    obj = ROOT / "vr180_convert_amd" / "csrc" / "kernels_jpegdec.o"
    assert obj.exists(), "kernels_jpegdec.o is built by __graft_entry__.build() / make"
    kernels = kernel_metadata(tmp_path, obj)
    assert len(kernels) == 8 and all("k_jdec_" in k[".name"] for k in kernels)
    bad = [(k[".name"], k[".private_segment_fixed_size"], k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for k in kernels
           if k[".private_segment_fixed_size"] or k[".sgpr_spill_count"] or k[".vgpr_spill_count"]]
    assert not bad, bad
    assert all(k[".wavefront_size"] == 64 for k in kernels)


# ---- device_decode plumbing -----------------------------------------------------------------------------------------------------------
def test_eligibility_and_exports():
    import vr180_convert_amd as V
    from vr180_convert_amd import jpeg_decode_device as J

    assert V.decode_jpeg_tensor is J.decode_jpeg_tensor and V.imread_tensor is J.imread_tensor and V.last_decode_report is J.last_decode_report
    assert J.eligible("a.jpg") and J.eligible(Path("b/a.JPEG")) and J.eligible("x.Jpeg")
    assert not J.eligible("a.png") and not J.eligible(None) and not J.eligible(np.zeros((4, 4, 3), np.uint8)) and not J.eligible("jpg")
    with pytest.raises(ValueError):
        J.decode_jpeg_tensor(b"\xff\xd8\xff\xd9", channels=2)
    with pytest.raises(ValueError):
        J.decode_jpeg_tensor(CASES["size_8x8_420"], subseq_bits=100)
    # refused by the parse, before any device is looked for
    with pytest.raises(NotImplementedError):
        J.decode_jpeg_tensor(DC.unsupported_cases()["progressive"])
    with pytest.raises(ValueError):
        J.decode_jpeg_tensor(DC.corrupt_cases()["no_eoi"][0])
    h, w, nc = J.probe(CASES["size_15x33_422"])
    assert (h, w, nc) == (15, 33, 3)


def test_read_inputs_sends_only_unsupported_and_damaged_files_to_the_host(tmp_path, monkeypatch, caplog):
    import logging

    from vr180_convert_amd import jpeg_decode_device as J

    def fake(path, **kw):
        name = Path(path).name
        if name == "p.jpg":
            raise NotImplementedError("progressive")
        if name == "bad.jpg":
            raise J.CorruptJPEG("damaged")
        if name == "gone.jpg":
            raise FileNotFoundError(name)
        if name == "bug.jpg":
            raise ValueError("an argument error")
        return "tensor of " + name

    monkeypatch.setattr(J, "imread_tensor", fake)
    arr = np.zeros((2, 2, 3), np.uint8)
    with caplog.at_level(logging.INFO, logger=J.LOG.name):
        got = J.read_inputs(["a.jpg", Path("p.jpg"), "bad.jpg", "gone.jpg", "x.png", arr])
    assert got[0] == "tensor of a.jpg" and got[1:5] == [Path("p.jpg"), "bad.jpg", "gone.jpg", "x.png"] and got[5] is arr
    levels = {r.getMessage().split(":")[0]: r.levelno for r in caplog.records}
    assert levels == {"p.jpg": logging.INFO, "bad.jpg": logging.WARNING, "gone.jpg": logging.WARNING}
    with pytest.raises(ValueError, match="argument"):
        J.read_inputs(["bug.jpg"])
    assert issubclass(J.CorruptJPEG, ValueError)
    with pytest.raises(J.CorruptJPEG):
        J.probe(DC.corrupt_cases()["dht_ac_all_codes_of_1_bit"][0])


def test_device_decode_plumbing_with_a_stubbed_decoder(tmp_path, monkeypatch):
    """eligible paths go to the device decoder, a file it reports unsupported goes to _io.imread as before, arrays and other suffixes
    never reach it, and with the flag off nothing changes"""
    import torch

    from vr180_convert_amd import _io, jpeg_decode_device, remapper

    decoded, host_reads = [], []

    def fake_decode(path, **kw):
        if "progressive" in Path(path).name:
            raise NotImplementedError("progressive")
        decoded.append(Path(path).name)
        return torch.zeros((4, 8 if "sbs" in Path(path).name else 4, 3), dtype=torch.uint8)

    monkeypatch.setattr(jpeg_decode_device, "imread_tensor", fake_decode)
    monkeypatch.setattr(_io, "imread", lambda p: host_reads.append(Path(p).name) or np.zeros((4, 4, 3), np.uint8))
    monkeypatch.setattr(_io, "imread_many", lambda paths: [host_reads.append(Path(p).name) or np.zeros((4, 4, 3), np.uint8)
                                                           if isinstance(p, (str, Path)) else p for p in paths])
    monkeypatch.setattr(_io, "imwrite", lambda p, a: True)
    monkeypatch.setattr(_io, "imwrite_many", lambda ps, ims: None)
    monkeypatch.setattr(remapper, "_to_device", lambda im, dev: im)
    monkeypatch.setattr(remapper, "_device", lambda device=None: torch.device("cpu"))
    monkeypatch.setattr(remapper, "_radius_for_pair", lambda *a: 1.0)
    seen = []
    monkeypatch.setattr(remapper, "apply_lr_tensors", lambda t, l, r, **k: seen.append((type(l).__name__, tuple(l.shape), tuple(r.shape))) or
                        torch.zeros((4, 8, 3), dtype=torch.uint8))
    for n in ("l.jpg", "r.JPEG", "progressive.jpg", "l.png", "sbs.jpg"):
        (tmp_path / n).write_bytes(b"")

    def lr(left, right, **kw):
        decoded.clear(), host_reads.clear(), seen.clear()
        remapper.apply_lr(None, left_path=left if isinstance(left, np.ndarray) else tmp_path / left,
                          right_path=right if isinstance(right, np.ndarray) else tmp_path / right, out_path=tmp_path / "o.png",
                          size_output=(4, 4), **kw)
        return list(decoded), list(host_reads)

    assert lr("l.jpg", "r.JPEG", device_decode=True) == (["l.jpg", "r.JPEG"], [])
    assert seen == [("Tensor", (4, 4, 3), (4, 4, 3))]
    assert lr("l.jpg", "r.JPEG") == ([], ["l.jpg", "r.JPEG"])                       # off by default
    assert lr("l.jpg", "r.JPEG", device_decode=False) == ([], ["l.jpg", "r.JPEG"])
    assert lr("l.jpg", "l.png", device_decode=True) == (["l.jpg"], ["l.png"])
    assert lr("progressive.jpg", "r.JPEG", device_decode=True) == (["r.JPEG"], ["progressive.jpg"])
    assert lr("sbs.jpg", "sbs.jpg", device_decode=True) == (["sbs.jpg"], [])        # one decode, two halves
    assert seen == [("Tensor", (4, 4, 3), (4, 4, 3))]
    assert lr(np.zeros((4, 4, 3), np.uint8), "r.JPEG", device_decode=True) == (["r.JPEG"], [])

    monkeypatch.setattr(remapper, "get_radius_smart", lambda r, ims: 1.0)
    monkeypatch.setattr(remapper, "remap_tensors", lambda *a, **k: None)
    monkeypatch.setattr(remapper.torch, "empty", lambda shape, dtype=None, device=None: torch.zeros(shape, dtype=torch.uint8))
    monkeypatch.setattr(remapper._hostpipe, "enabled", lambda *a: False)  # (the pipelined host route needs a device)

    def s(names, **kw):
        decoded.clear(), host_reads.clear()
        remapper.apply(None, in_paths=[tmp_path / n for n in names], out_paths=[tmp_path / f"o{i}.png" for i in range(len(names))],
                       size_output=(4, 4), **kw)
        return list(decoded), list(host_reads)

    assert s(["l.jpg", "progressive.jpg", "l.png"], device_decode=True) == (["l.jpg"], ["progressive.jpg", "l.png"])
    assert s(["l.jpg", "progressive.jpg", "l.png"]) == ([], ["l.jpg", "progressive.jpg", "l.png"])


def test_cli_flag_reaches_apply_and_apply_lr(tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from vr180_convert_amd import _io, cli, remapper, synth

    seen = []
    monkeypatch.setattr(remapper, "apply_lr", lambda *a, **k: seen.append(("lr", k.get("device_decode"), k.get("device_jpeg"))))
    monkeypatch.setattr(remapper, "apply", lambda *a, **k: seen.append(("s", k.get("device_decode"), k.get("device_jpeg"))))
    img = tmp_path / "a.png"
    _io.imwrite(img, synth.pattern(64, 64))
    run = CliRunner().invoke
    base = ["--radius", "max", "--size", "32x32"]
    assert run(cli.app, ["lr", str(img), str(img), *base, "--device-decode", "--out-path", str(tmp_path / "o.jpg")]).exit_code == 0
    assert run(cli.app, ["lr", str(img), str(img), *base, "--out-path", str(tmp_path / "o.jpg")]).exit_code == 0
    assert run(cli.app, ["s", str(img), *base, "--device-decode", "--device-jpeg", "--out-path", str(tmp_path / "o.jpg")]).exit_code == 0
    assert run(cli.app, ["s", str(img), *base, "--out-path", str(tmp_path / "o.jpg")]).exit_code == 0
    assert seen == [("lr", True, None), ("lr", None, None), ("s", True, True), ("s", None, None)]


def test_cli_devfm_and_apply_lr_share_one_decode(tmp_path, monkeypatch):
    """``--automatch devfm --device-decode``: the pair is decoded once; the matcher and apply_lr get the same tensors"""
    from typer.testing import CliRunner

    from vr180_convert_amd import cli, jpeg_decode_device, remapper

    calls, seen = [], {}
    monkeypatch.setattr(jpeg_decode_device, "read_inputs", lambda items, **k: calls.append(list(items)) or [("decoded", Path(q).name) for q in items])
    monkeypatch.setattr(cli, "calibrated_pair", lambda chain, automatch, left, right, radius, match=None: seen.update(match=(left, right)) or chain)
    monkeypatch.setattr(remapper, "apply_lr", lambda chain, **k: seen.update(lr=(k["left_path"], k["right_path"]), flag=k.get("device_decode")))
    a, b = tmp_path / "a.jpg", tmp_path / "b.jpg"
    a.write_bytes(b""), b.write_bytes(b"")
    base = ["--radius", "max", "--size", "32x32", "--out-path", str(tmp_path / "o.png")]
    r = CliRunner().invoke(cli.app, ["lr", str(a), str(b), *base, "--automatch", "devfm", "--device-decode"])
    assert r.exit_code == 0, (r.output, r.exception)
    assert calls == [[a, b]] and seen["match"] == seen["lr"] == (("decoded", "a.jpg"), ("decoded", "b.jpg")) and seen["flag"] is True
    calls.clear()
    r = CliRunner().invoke(cli.app, ["lr", str(a), str(b), *base, "--automatch", "devfm"])
    assert r.exit_code == 0 and calls == [] and seen["match"] == seen["lr"] == (a, b) and seen["flag"] is None
