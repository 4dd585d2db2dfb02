"""The device decoder of progressive JPEG files without a GPU: the restatement (jpgprog_ref.py) against Pillow and against its own plain
decoder; the product's jpegprog_core.hpp / jpegprog_host.hpp run on the host, in a sequential copy of the kernels' decomposition,
against the restatement value for value; the same build under the address and undefined-behaviour sanitizers as a stand-alone
program; the codes of incomplete and illegal scripts; the option's default; the resource budget of kernels_jpegprog.o; the plumbing of
``device_decode_progressive``."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jpgdec_ref as D
import jpgdmg_cases as M
import jpgprog_cases as PCS
import jpgprog_ref as P

ROOT = Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "host_jpegdec_prog" / "jpegprog_emul.hip"
CASES = PCS.supported_cases()


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_jpegdec_prog") / "libjpegprog_emul.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-fno-fast-math", "-o", str(out),
                    str(HARNESS)], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(out))
    vp, u32 = C.c_void_p, C.c_uint32
    lib.jprog_emul_info.argtypes = [C.c_char_p, C.c_uint64, vp]
    lib.jprog_emul_decode.argtypes = [C.c_char_p, C.c_uint64, u32, C.c_int, vp, u32, vp, vp, u32, vp, vp, vp, vp]
    return lib


def _emul_info(lib, data):
    info = np.zeros(8, np.int32)
    return lib.jprog_emul_info(data, len(data), info.ctypes.data), info


def _emul_decode(lib, data, S, cn=3):
    rc, info = _emul_info(lib, data)
    assert rc == 0
    h, w, scans, nblocks = int(info[0]), int(info[1]), int(info[5]), int(info[6])
    cap = len(data) * 8 // 256 + 70000
    after = np.zeros((scans, nblocks, 64), np.int16)
    states, counts = np.zeros((cap, 5), np.uint32), np.zeros(cap, np.uint32)
    rounds, nsub, report = np.zeros(scans, np.uint32), np.zeros(scans, np.uint32), np.zeros(5, np.uint32)
    px = np.zeros((h, w, cn), np.uint8)
    rc = lib.jprog_emul_decode(data, len(data), S, cn, after.ctypes.data, scans, states.ctypes.data, counts.ctypes.data, cap,
                               rounds.ctypes.data, nsub.ctypes.data, report.ctypes.data, px.ctypes.data)
    n = int(report[1])
    return rc, after, states[:n], counts[:n], rounds, nsub, report, px


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_pillow_and_its_plain_decoder(name):
    """On every supported case, at both subsequence sizes: largest difference to Pillow 0, differing samples 0 -- the coefficients are
    exact integers and the pixel stage is the sequential decoder's, proven equal already: a condition, not a tolerance.  At the first
    size ``P.decode(check=True)`` also holds the iteration to the plain decoder scan by scan: the same coefficients, the same state
    wherever the plain decoder passes a subsequence's first bit.  Every file decodes in Pillow, the writer's among them."""
    data = CASES[name]
    want = PCS.pillow_pixels(data)
    for i, S in enumerate(PCS.SUBSEQ):
        r = P.decode(data, S, check=i == 0)
        diff = np.abs(r.pixels.astype(int) - want.astype(int))
        assert int(diff.max()) == 0 and int((diff != 0).sum()) == 0, (name, S)
        assert all(rd <= len(e) + 1 for rd, e in zip(r.scan_rounds, r.entries)) and r.rounds == sum(r.scan_rounds)
        assert np.array_equal(r.coef, PCS.reference(name, PCS.SUBSEQ[0]).coef)


def test_case_list_sits_on_the_boundaries_it_is_for():
    kinds = {n: [sc.kind for sc in PCS.reference(n, 256).info.scans] for n in CASES}
    assert all(len(set(k)) == 4 for n, k in kinds.items() if n.startswith("pil_"))        # Pillow's script has all four scan kinds
    assert set(kinds["w_selection_only_420"]) == {P.DC_FIRST, P.AC_FIRST}
    r = PCS.reference("w_dc_per_component_422", 256)
    assert [sc.ni for sc in r.info.scans[:3]] == [True] * 3 and r.info.scans[1].nunits < r.info.nmcu * r.info.ny  # narrower than the MCUs' grid
    assert len(PCS.reference("w_one_coefficient_bands", 256).info.scans) == 64
    assert [sc.Al for sc in PCS.reference("w_al2_444", 256).info.scans if sc.kind == P.AC_REFINE] == [1, 1, 1, 0, 0, 0]
    assert len({sc.restart for sc in PCS.reference("w_dri_changed_420", 256).info.scans}) == 4
    assert any(sc.nseg == sc.nmcu > 1 for sc in PCS.reference("pil_128_dri1", 256).info.scans)
    # an end-of-band run of 32767 blocks: the EOB14 symbol with fourteen 1 bits behind it, and one step ends them all
    r = PCS.reference("w_eobrun_32767", 1024)
    assert r.info.scans[1].nunits == 32768 and max(r.counts[1]) >= 32767
    # one end-of-band run over many subsequences in a refinement scan: its correction bits
    r = PCS.reference("w_correction_run", 256)
    assert len(r.entries[3]) > 4 and any(e[3] > 1 for e in r.entries[3][1:]) and r.scan_rounds[3] > 2
    # ... and a run whose blocks take no bits at all (a flat field) in a first scan and in a refinement scan
    r = PCS.reference("pil_flat_one_block", 256)
    assert all(max(c) > 256 for sc, c in zip(r.info.scans, r.counts) if sc.kind >= P.AC_FIRST)
    # long codes and slow synchronisation
    assert max(PCS.reference("pil_noise_q100_gray", 256).scan_rounds) > 50


def test_unsupported_and_corrupt_files_by_the_restatement():
    for name, data in PCS.unsupported_cases().items():
        with pytest.raises(D.Unsupported):
            P.decode(data)
    for name, (data, by_parse) in PCS.corrupt_cases().items():
        with pytest.raises(D.Corrupt):
            (P.parse if by_parse else P.decode)(data)
        if not by_parse:
            P.parse(data)
    with pytest.raises(D.Corrupt, match="scan 2"):
        P.decode(PCS.corrupt_cases()[PCS.TRUNCATED][0])


# ---- the product's headers on the host ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_product_host_code_equals_restatement(emul, name):
    """coefficients behind every scan, entry states, block counts, rounds per scan and pixels, at both subsequence sizes"""
    data = CASES[name]
    for S in PCS.SUBSEQ:
        ref = PCS.reference(name, S)
        rc, after, states, counts, rounds, nsub, report, px = _emul_decode(emul, data, S)
        assert rc == 0, (name, S, rc)
        assert list(report[:3]) == [ref.scans, ref.subsequences, ref.rounds]
        assert list(rounds) == ref.scan_rounds and list(nsub) == [len(e) for e in ref.entries]
        assert np.array_equal(after, np.stack(ref.after)), (name, S)
        assert [tuple(int(v) for v in s) for s in states] == [e for es in ref.entries for e in es]
        assert list(counts) == [c for cs in ref.counts for c in cs]
        assert np.array_equal(px, ref.pixels), (name, S)
    if P.parse(data).nc == 1:
        assert np.array_equal(_emul_decode(emul, data, 0, 1)[-1][..., 0], P.decode(data, 0, 1, check=False).pixels)


def test_incomplete_and_illegal_scripts_on_the_host_build(emul):
    """the specified codes without a device: 1 unsupported, 2 corrupt by the parse, 3 corrupt by the last pass"""
    for name, data in PCS.unsupported_cases().items():
        assert _emul_info(emul, data)[0] == 1, name
    for name, (data, by_parse) in PCS.corrupt_cases().items():
        rc, _ = _emul_info(emul, data)
        assert rc == (2 if by_parse else 0), name
        if not by_parse:
            out = _emul_decode(emul, data, 256)
            assert out[0] == 3 and int(out[6][4]) == 2, name   # the earliest bad scan: the third


def test_standalone_sanitizer_run(tmp_path):
    """the host build as a program of its own under the address and undefined-behaviour sanitizers: the supported cases, the unsupported
    and the corrupt ones, the truncations of one file and every damaged scan of tests/jpgdmg_cases.py, from heap copies of the files'
    exact sizes; any report fails the run"""
    exe = tmp_path / "jpegprog_san"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fno-fast-math", "-DJPROG_MAIN", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(HARNESS)], check=True,
                   capture_output=True, timeout=600)
    files = {}
    for group, cases in (("ok", CASES), ("unsup", PCS.unsupported_cases()), ("bad", {n: d for n, (d, _) in PCS.corrupt_cases().items()})):
        for name, data in cases.items():
            p = tmp_path / f"{group}_{name}.jpg"
            p.write_bytes(data)
            files[str(p)] = group
    base = CASES["w_dri_changed_420"]
    for n in list(range(0, 400, 7)) + list(range(400, len(base), 11)):
        p = tmp_path / f"cut_{n}.jpg"
        p.write_bytes(base[:n])
        files[str(p)] = "cut"
    # the damaged scans of tests/jpgdmg_cases.py, which do reach the entropy decoder: the exit code is the restatement's class
    for k, x in enumerate(M.progressive_cases()):
        p = tmp_path / f"dmg_{k}.jpg"
        p.write_bytes(x.data)
        files[str(p)] = M.verdict(x.name, 256, True).what
    r = subprocess.run([str(exe), *files], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 * len(files)
    for line in lines:
        path, rc = line.split(" S=")[0], int(line.split("rc=")[1].split()[0])
        want = {"ok": (0,), "unsup": (1,), "bad": (2, 3), "cut": (2, 3), "decoded": (0,), "unsupported": (1,), "parse": (2,),
                "refused": (3,)}[files[path]]
        assert rc in want, line


# ---- the library without a device -----------------------------------------------------------------------------------------------------
def test_prog_info_and_argument_checks_without_device(product_lib):
    from vr180_convert_amd import _abi

    lib = product_lib
    info = _abi.JpegProgInfo()
    for name, data in CASES.items():
        s = P.parse(data)
        assert lib.v1c_jpeg_prog_info(data, len(data), C.byref(info)) == 0, name
        assert [info.height, info.width, info.components, info.h_samp, info.v_samp, info.scans] == [s.h, s.w, s.nc, s.hs, s.vs, len(s.scans)]
    for name, data in PCS.unsupported_cases().items():
        assert lib.v1c_jpeg_prog_info(data, len(data), C.byref(info)) == -2, name
    assert b"byte" in lib.v1c_last_error()
    for name, (data, by_parse) in PCS.corrupt_cases().items():
        assert lib.v1c_jpeg_prog_info(data, len(data), C.byref(info)) == (-5 if by_parse else 0), name
    assert lib.v1c_jpeg_prog_info(None, 10, C.byref(info)) == -1 and lib.v1c_jpeg_prog_info(b"abcd", 4, None) == -1
    assert lib.v1c_jpeg_prog_info(b"", 0, C.byref(info)) == -5

    out = np.zeros(1 << 16, np.uint8)  # stands in for the device pointer: validation fails before any device call
    data = CASES["pil_420_q90"]

    def call(file=data, size=len(data), dst=out.ctypes.data, pitch=47 * 3, cn=3, S=0, cap=0):
        return lib.v1c_jpeg_prog_decode(0, None, file, size, dst, pitch, cn, S, None, None, cap)

    def err():
        return lib.v1c_last_error().decode()

    assert call(file=None) == -1 and "NULL" in err() and call(dst=None) == -1
    assert call(cn=2) == -1 and "out_cn" in err()
    assert call(cn=1) == -1 and "one component" in err()
    assert call(S=128) == -1 and "subseq_bits" in err() and call(S=300) == -1
    assert call(pitch=50) == -1 and "pitch" in err()
    assert call(cap=3) == -1 and "scan_cap" in err()
    for name, d in PCS.unsupported_cases().items():
        assert call(file=d, size=len(d)) == -2, name
    for name, (d, by_parse) in PCS.corrupt_cases().items():
        if by_parse:
            assert call(file=d, size=len(d)) == -5, name


def test_with_the_option_off_a_progressive_file_is_refused_as_ever(product_lib):
    """the sequential entry points keep their answer for every progressive file, and ``decode_jpeg_tensor`` without ``progressive``
    raises what it raised, before it looks for a device"""
    from vr180_convert_amd import jpeg_decode_device as J

    info = (C.c_int32 * 6)()
    for name, data in CASES.items():
        assert product_lib.v1c_jpeg_decode_info(data, len(data), info) == -2, name
        assert b"progressive, lossless or arithmetic" in product_lib.v1c_last_error()
    data = CASES["pil_420_q90"]
    with pytest.raises(NotImplementedError, match="progressive, lossless or arithmetic"):
        J.decode_jpeg_tensor(data)
    with pytest.raises(NotImplementedError, match="progressive, lossless or arithmetic"):
        J.decode_jpeg_tensor(data, progressive=False)
    # with it on, what the progressive parse refuses is refused by the host alone too, and a sequential file is not its business
    with pytest.raises(NotImplementedError, match="unfinished"):
        J.decode_jpeg_tensor(PCS.unsupported_cases()["incomplete_band"], progressive=True)
    with pytest.raises(J.CorruptJPEG):
        J.decode_jpeg_tensor(PCS.corrupt_cases()["dc_scan_with_band"][0], progressive=True)
    assert J.probe_progressive(data) == (33, 47, 3, 10)
    with pytest.raises(NotImplementedError, match="sequential"):
        J.probe_progressive(PCS.unsupported_cases()["sequential"])
    assert J._is_progressive(data) and not J._is_progressive(PCS.unsupported_cases()["sequential"]) and not J._is_progressive(b"\xff\xd8\xff")


def test_kernels_jpegprog_use_no_scratch_and_spill_nothing(tmp_path, product_lib):
    from test_resource_budget import kernel_metadata

    obj = ROOT / "vr180_convert_amd" / "csrc" / "kernels_jpegprog.o"
    assert obj.exists(), "kernels_jpegprog.o is built by __graft_entry__.build() / make"
    kernels = kernel_metadata(tmp_path, obj)
    assert len(kernels) == 6 and all("k_jprog_" in k[".name"] for k in kernels)
    bad = [(k[".name"], k[".private_segment_fixed_size"], k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for k in kernels
           if k[".private_segment_fixed_size"] or k[".sgpr_spill_count"] or k[".vgpr_spill_count"]]
    assert not bad, bad
    assert all(k[".wavefront_size"] == 64 for k in kernels)


# ---- device_decode_progressive plumbing -----------------------------------------------------------------------------------------------
def test_read_inputs_passes_the_option_on(tmp_path, monkeypatch):
    from vr180_convert_amd import jpeg_decode_device as J

    seq, prog = tmp_path / "a.jpg", tmp_path / "b.jpg"
    seq.write_bytes(PCS.unsupported_cases()["sequential"]), prog.write_bytes(CASES["pil_420_q90"])
    calls = []

    def fake_single(path, *, device=None, channels=3, subseq_bits=None, progressive=False):
        calls.append((Path(path).name, progressive))
        if Path(path) == prog and not progressive:
            raise NotImplementedError("progressive, lossless or arithmetic")
        return f"tensor of {Path(path).name}"

    def fake_batch(paths, *, device=None, errors="raise", **kw):
        calls.append(("batch", [Path(p).name for p in paths]))
        return [NotImplementedError("progressive") if Path(p) == prog else f"tensor of {Path(p).name}" for p in paths]

    monkeypatch.setattr(J, "imread_tensor", fake_single)
    monkeypatch.setattr(J, "imread_tensors", fake_batch)
    assert J.read_inputs([seq, prog]) == ["tensor of a.jpg", prog]
    assert J.read_inputs([seq, prog], progressive=True) == ["tensor of a.jpg", "tensor of b.jpg"]
    calls.clear()
    assert J.read_inputs([seq, prog], batch=True) == ["tensor of a.jpg", prog] and calls == [("batch", ["a.jpg", "b.jpg"])]
    calls.clear()
    # the batch refuses the progressive file as it does now; a single call behind it takes it
    assert J.read_inputs([seq, prog], batch=True, progressive=True) == ["tensor of a.jpg", "tensor of b.jpg"]
    assert calls == [("batch", ["a.jpg", "b.jpg"]), ("b.jpg", True)]


def test_apply_and_cli_pass_the_option_on(tmp_path, monkeypatch):
    import inspect

    from typer.testing import CliRunner

    from vr180_convert_amd import cli, remapper

    for f in (remapper.apply, remapper.apply_lr):
        assert inspect.signature(f).parameters["device_decode_progressive"].default is False
    seen = []
    monkeypatch.setattr("vr180_convert_amd.jpeg_decode_device.read_inputs", lambda items, **kw: seen.append(kw) or list(items))
    remapper._decode_on_device(["x.jpg"], None, True)
    remapper._decode_on_device(["x.jpg"], None, "batch", True)
    assert seen == [{"device": None}, {"device": None, "batch": True, "progressive": True}]
    got = {}
    monkeypatch.setattr(remapper, "apply", lambda *a, **kw: got.update(kw))
    src = tmp_path / "in.jpg"
    src.write_bytes(CASES["pil_420_q90"])
    r = CliRunner().invoke(cli.app, ["s", str(src), "--device-decode", "--device-decode-progressive", "--out-path", str(tmp_path / "o.png")])
    assert r.exit_code == 0, r.output
    assert got["device_decode"] is True and got["device_decode_progressive"] is True
    got.clear()
    r = CliRunner().invoke(cli.app, ["s", str(src), "--device-decode", "--out-path", str(tmp_path / "o.png")])
    assert r.exit_code == 0 and "device_decode_progressive" not in got
