"""The device decoder of progressive JPEG files on the MI355X: every case of tests/jpgprog_cases.py against the restatement
(tests/jpgprog_ref.py) byte for byte -- pixels, rounds per scan, the report --, which test_jpegprog_host.py holds to Pillow with 0
differing samples; the C ABI's edges (pitched and unaligned outputs, two streams, a damaged scan, stream capture); and
``device_decode_progressive`` in apply_lr, apply with a batch, and the command line."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import jpgdec_cases as DC
import jpgprog_cases as PCS

pytestmark = pytest.mark.gpu
CASES = PCS.supported_cases()


@pytest.fixture(scope="module")
def V():
    import vr180_convert_amd as V

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    return V


@pytest.fixture(scope="module")
def lib(V):
    from vr180_convert_amd import _native

    return _native.lib()


def decode(lib, data, S, out, cn=3, stream=None, scans=0):
    """through the C ABI into the (h, w[, cn]) device tensor ``out`` (rows may be pitched): (return code, report, rounds per scan)"""
    from vr180_convert_amd import _abi

    rep = _abi.JpegProgReport()
    per = (C.c_uint32 * max(scans, 1))()
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    rc = lib.v1c_jpeg_prog_decode(0, st, data, len(data), out.data_ptr(), out.stride(0), cn, S, C.byref(rep), per, scans)
    return rc, rep, list(per)[:scans]


@pytest.mark.parametrize("name", list(CASES))
def test_case_equals_restatement(V, name):
    """pixels, rounds per scan and the report at both subsequence sizes: 0 differing bytes"""
    from vr180_convert_amd import jpeg_decode_device as J

    for S in PCS.SUBSEQ:
        ref = PCS.reference(name, S)
        got = J.decode_jpeg_tensor(CASES[name], subseq_bits=S, progressive=True).cpu().numpy()
        rep = J.last_decode_report()
        print(name, S, "differing bytes", int((got != ref.pixels).sum()), "rounds", rep["scan_rounds"], "want", ref.scan_rounds)
        assert got.shape == ref.pixels.shape and int((got != ref.pixels).sum()) == 0, (name, S)
        assert rep == dict(segments=ref.segments, subsequences=ref.subsequences, rounds=ref.rounds, path="device", scans=ref.scans,
                           scan_rounds=ref.scan_rounds), (name, S)


def test_sequential_files_behave_as_without_the_option(V):
    from vr180_convert_amd import jpeg_decode_device as J

    data = DC.supported_cases()["size_17x17_420"]
    a = J.decode_jpeg_tensor(data).cpu().numpy()
    ra = J.last_decode_report()
    b = J.decode_jpeg_tensor(data, progressive=True).cpu().numpy()
    assert np.array_equal(a, b) and J.last_decode_report() == ra and "scans" not in ra


@pytest.mark.parametrize("name", ["pil_13x17_420", "w_al2_444"])
def test_pitched_and_odd_offset_output(lib, name):
    want = PCS.reference(name, 256).pixels
    h, w = want.shape[:2]
    whole = torch.full((h, 3 * w + 5, 3), 0x5A, dtype=torch.uint8, device="cuda")
    assert decode(lib, CASES[name], 256, whole[:, :w])[0] == 0, lib.v1c_last_error()
    got = whole.cpu().numpy()
    assert np.array_equal(got[:, :w], want) and (got[:, w:] == 0x5A).all()
    flat = torch.full((h * (3 * w + 7) + 1,), 0x5A, dtype=torch.uint8, device="cuda")
    view = flat[1:].view(h, 3 * w + 7)[:, :3 * w].unflatten(1, (w, 3))  # behind an odd byte offset, with an odd pitch: no row is aligned
    assert view.data_ptr() % 2 == 1 and decode(lib, CASES[name], 256, view)[0] == 0
    got = flat.cpu().numpy()[1:].reshape(h, 3 * w + 7)
    assert np.array_equal(got[:, :3 * w].reshape(h, w, 3), want) and (got[:, 3 * w:] == 0x5A).all() and flat[0].item() == 0x5A


def test_one_channel(V):
    from vr180_convert_amd import jpeg_decode_device as J

    for name in ("pil_gray_q90", "w_al3_gray_dri"):
        got = J.decode_jpeg_tensor(CASES[name], channels=1, progressive=True)
        want = PCS.reference(name, 0).pixels
        assert got.shape == want.shape[:2] and np.array_equal(got.cpu().numpy(), want[..., 0])
    with pytest.raises(ValueError):
        J.decode_jpeg_tensor(CASES["pil_420_q90"], channels=1, progressive=True)


def test_two_streams_back_to_back(lib):
    """two different files on two streams, no device-wide synchronize in between"""
    na, nb = "pil_422_q100", "w_dri_changed_420"
    wa, wb = PCS.reference(na, 256).pixels, PCS.reference(nb, 256).pixels
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(3):
        a = torch.zeros(wa.shape, dtype=torch.uint8, device="cuda")
        b = torch.zeros(wb.shape, dtype=torch.uint8, device="cuda")
        torch.cuda.current_stream().synchronize()  # (the fills above: on the default stream)
        assert decode(lib, CASES[na], 256, a, stream=s1)[0] == 0
        assert decode(lib, CASES[nb], 256, b, stream=s2)[0] == 0
        outs += [a, b]
    s1.synchronize(), s2.synchronize()
    assert all(np.array_equal(o.cpu().numpy(), wa) for o in outs[0::2])
    assert all(np.array_equal(o.cpu().numpy(), wb) for o in outs[1::2])


def test_truncated_third_scan_is_reported_and_the_next_decode_is_right(V, lib):
    """(the stand-alone sanitizer run of tests/test_jpegprog_host.py shows that truncated input keeps every read in bounds)"""
    from vr180_convert_amd import jpeg_decode_device as J

    data = PCS.corrupt_cases()[PCS.TRUNCATED][0]
    with pytest.raises(J.CorruptJPEG, match="scan 2"):
        J.decode_jpeg_tensor(data, progressive=True)
    out = torch.zeros((64, 96, 3), dtype=torch.uint8, device="cuda")
    rc, rep, _ = decode(lib, data, 256, out)
    assert rc == -5 and rep.error_scan == 2 and b"damaged" in lib.v1c_last_error()
    name = "pil_13x17_422"
    want = PCS.reference(name, 256).pixels
    out = torch.zeros(want.shape, dtype=torch.uint8, device="cuda")
    rc, rep, rounds = decode(lib, CASES[name], 256, out, scans=10)
    assert rc == 0 and rounds == PCS.reference(name, 256).scan_rounds and np.array_equal(out.cpu().numpy(), want)


def test_refused_under_stream_capture(lib):
    """the host reads a flag between the rounds: under capture the call is refused before it does anything"""
    name = "pil_8x8_420"
    out = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out.zero_()
            rc, _, _ = decode(lib, CASES[name], 0, out, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    assert rc == -2 and b"graph" in lib.v1c_last_error()
    assert decode(lib, CASES[name], 0, out)[0] == 0
    assert np.array_equal(out.cpu().numpy(), PCS.reference(name).pixels)


# ---- through apply_lr, apply and the command line ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain():
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder, PolynomialScaler

    return EquirectangularEncoder() * PolynomialScaler([0, 1, -0.1]) * FisheyeDecoder("equidistant")


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """two progressive 256 x 256 JPEG files of fisheye-like discs by Pillow, and a sequential one"""
    from vr180_convert_amd.synth import noise_disc

    d = tmp_path_factory.mktemp("jpegprog")
    left, right = (np.pad(noise_disc(208, 208, f), ((24, 24), (24, 24), (0, 0))) for f in (0, 1))
    (d / "l.jpg").write_bytes(DC.pillow(left, 92, "420", progressive=True))
    (d / "r.jpeg").write_bytes(DC.pillow(right, 92, "444", progressive=True))
    (d / "s.jpg").write_bytes(DC.pillow(right, 92, "422"))
    return d


def test_apply_lr_keeps_a_progressive_pair_on_the_device(V, chain, pair, tmp_path, monkeypatch):
    from vr180_convert_amd import _io

    kw = dict(size_output=(256, 256), interpolation=1, radius=120.0)
    l, r = (_io.imread(pair / n) for n in ("l.jpg", "r.jpeg"))  # the host reader's arrays
    V.apply_lr(chain, left_path=l, right_path=r, out_path=tmp_path / "want.npy", **kw)
    host_reads = []
    real = _io.imread
    monkeypatch.setattr(_io, "imread", lambda p: host_reads.append(Path(p).name) or real(p))
    V.apply_lr(chain, left_path=pair / "l.jpg", right_path=pair / "r.jpeg", out_path=tmp_path / "got.npy", device_decode=True,
               device_decode_progressive=True, **kw)
    want = np.load(tmp_path / "want.npy")
    assert host_reads == [] and want.any() and np.array_equal(np.load(tmp_path / "got.npy"), want)
    # without the new option the files go to the host reader, as before
    V.apply_lr(chain, left_path=pair / "l.jpg", right_path=pair / "r.jpeg", out_path=tmp_path / "got2.npy", device_decode=True, **kw)
    assert sorted(host_reads) == ["l.jpg", "r.jpeg"] and np.array_equal(np.load(tmp_path / "got2.npy"), want)


def test_apply_with_a_batch_of_a_mixed_list(V, chain, pair, tmp_path, monkeypatch):
    from vr180_convert_amd import _io
    from vr180_convert_amd import jpeg_decode_device as J

    host_reads = []
    real = _io.imread
    monkeypatch.setattr(_io, "imread", lambda p: host_reads.append(Path(p).name) or real(p))
    kw = dict(size_output=(256, 256), interpolation=1, radius=120.0)
    names = ["s.jpg", "l.jpg", "r.jpeg"]
    outs = V.apply(chain, in_paths=[pair / n for n in names], device_decode="batch", device_decode_progressive=True, **kw)
    assert host_reads == [] and J.last_batch_report()["files"][1] is None and J.last_decode_report()["scans"] == 10
    want = V.apply(chain, in_paths=[real(pair / n) for n in names], **kw)
    for o, w in zip(outs, want):
        assert w.any() and np.array_equal(o.cpu().numpy(), w)


def test_cli_device_decode_progressive(V, pair, tmp_path):
    from typer.testing import CliRunner

    from vr180_convert_amd import cli
    from vr180_convert_amd import jpeg_decode_device as J

    J._last.clear()
    r = CliRunner().invoke(cli.app, ["s", str(pair / "l.jpg"), "--device-decode", "--device-decode-progressive", "--size", "256x256",
                                     "--out-path", str(tmp_path / "cli.png")])
    assert r.exit_code == 0, r.output
    assert J.last_decode_report().get("scans") == 10
    r = CliRunner().invoke(cli.app, ["s", str(pair / "l.jpg"), "--size", "256x256", "--out-path", str(tmp_path / "host.png")])
    assert r.exit_code == 0, r.output
    assert (tmp_path / "cli.png").stat().st_size > 1000 and (tmp_path / "host.png").read_bytes() == (tmp_path / "cli.png").read_bytes()
