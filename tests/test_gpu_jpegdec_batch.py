"""The batched device JPEG decoder on the MI355X (``decode_jpeg_tensors`` / ``v1c_jpeg_decode_batch``): files of different size,
subsampling, tables and restart interval in shared launches and shared rounds, against the single call on the same device and against
the restatement (jpgdec_ref.py), sample for sample.  The shapes a flat work list can go wrong at are in tests/jpgdec_cases.py: files of
one subsequence next to files of four workgroups, a file of one MCU, last workgroups that are partial in every list.
tests/test_jpegdec_batch_host.py runs the same batches through the host build of the same decomposition."""
import ctypes as C
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch

import jpgdec_cases as DC

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
DOCS_JPG = ROOT / "tests" / "golden" / "ref_docs" / "test.jpg"
CASES = {**DC.supported_cases(), **DC.extreme_cases()}
NOISE, WIDE = "noise_q100_420", "noise_q100_444"   # the most rounds at 256 bits (232); the most subsequences (785: four workgroups)
SPREAD = ["size_8x8_444", "flat_420", NOISE, "size_17x17_420", WIDE, "quality_1"]


class Report(C.Structure):
    _fields_ = [("segments", C.c_uint32), ("subsequences", C.c_uint32), ("rounds", C.c_uint32), ("reserved", C.c_uint32),
                ("error_pos", C.c_uint64)]


@pytest.fixture(scope="module")
def V():
    import vr180_convert_amd as V

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    return V


@pytest.fixture(scope="module")
def singles(V):
    """(tensor on the host, report) of ``decode_jpeg_tensor`` per (name, subseq_bits): computed once, shared, never changed"""
    cache = {}

    def get(name, S):
        if (name, S) not in cache:
            t = V.decode_jpeg_tensor(CASES[name], subseq_bits=S).cpu().numpy()
            t.setflags(write=False)
            cache[name, S] = (t, V.last_decode_report())
        return cache[name, S]

    return get


def check_batch(V, singles, names, S, **kw):
    """the batch of ``names`` equals the single calls and the restatement file by file; returns last_batch_report()"""
    got = V.decode_jpeg_tensors([CASES[n] for n in names], subseq_bits=S, **kw)
    rep = V.last_batch_report()
    assert len(got) == len(names) == len(rep["files"])
    for n, t, r in zip(names, got, rep["files"]):
        want, single = singles(n, S)
        t = t.cpu().numpy()
        assert np.array_equal(t, want), (n, int((t != want).sum()))
        assert np.array_equal(t, DC.reference(n, 256).pixels), n
        assert r == single, n
    return rep


@pytest.mark.parametrize("S", [256, 1024])
def test_mixed_batch_equals_the_single_calls_and_the_restatement(V, singles, S):
    names = list(CASES)
    rep = check_batch(V, singles, names, S)
    assert rep["chunks"] == 1 and rep["batch_rounds"] == max(r["rounds"] for r in rep["files"])
    if S == 256:
        assert [r["subsequences"] for r in rep["files"]] == [DC.reference(n, 256).subsequences for n in names]
    rep = check_batch(V, singles, names[::-1], S)
    assert rep["batch_rounds"] == max(r["rounds"] for r in rep["files"])


def test_convergence_spread(V, singles):
    """files that are quiet after a few rounds rest for two hundred more beside the noise file, and are still exact at the end"""
    rep = check_batch(V, singles, SPREAD, 256)
    rounds = [r["rounds"] for r in rep["files"]]
    assert rep["batch_rounds"] == max(rounds) == rounds[2] > 150 and sorted(rounds)[-3] <= 8


def test_damaged_and_unsupported_files_in_the_middle(V, singles):
    from vr180_convert_amd import jpeg_decode_device as J

    good = ["size_17x17_420", WIDE, "dri1_444", "flat_gray_200"]
    items = [CASES[good[0]], CASES[good[1]], DC.corrupt_cases()[DC.TRUNCATED][0], DC.unsupported_cases()["progressive"], CASES[good[2]],
             DC.corrupt_cases()["rst1_for_rst0"][0], DC.corrupt_cases()["one_block_too_few"][0], CASES[good[3]]]
    got = V.decode_jpeg_tensors(items, subseq_bits=256, errors="return")
    rep = V.last_batch_report()
    assert isinstance(got[2], J.CorruptJPEG) and "bit" in str(got[2]) and isinstance(got[3], NotImplementedError)
    assert isinstance(got[5], J.CorruptJPEG) and "byte" in str(got[5]) and isinstance(got[6], J.CorruptJPEG)
    for i, n in zip((0, 1, 4, 7), good):
        want, single = singles(n, 256)
        assert np.array_equal(got[i].cpu().numpy(), want) and rep["files"][i] == single, n
    assert [rep["files"][i] for i in (2, 3, 5, 6)] == [None] * 4 and rep["chunks"] == 1
    with pytest.raises(J.CorruptJPEG, match="bit"):
        V.decode_jpeg_tensors(items, subseq_bits=256)
    # ... and the next batch is right
    check_batch(V, singles, good, 256)


def test_chunks(V, singles):
    names = ["size_17x17_420", WIDE, "dri1_444", "flat_420", NOISE, "size_8x8_gray", "midrow_420_r3"]
    rep = check_batch(V, singles, names, 256, max_workspace_bytes=1)  # below every file: every file a chunk of its own
    rounds = [r["rounds"] for r in rep["files"]]
    assert rep["chunks"] == len(names) and rep["batch_rounds"] == sum(rounds)
    rep = check_batch(V, singles, names, 256, max_workspace_bytes=300_000)  # (the two noise files take about 170 KB and 90 KB)
    assert 1 < rep["chunks"] < len(names) and max(rounds) < rep["batch_rounds"] < sum(rounds)
    assert check_batch(V, singles, names, 256, max_workspace_bytes=1 << 30)["chunks"] == 1


def test_a_batch_of_one_equals_the_single_call(V, singles):
    for n in ("size_8x8_444", WIDE, "dri1_gray"):
        for S in (256, 1024):
            rep = check_batch(V, singles, [n], S)
            assert rep["batch_rounds"] == rep["files"][0]["rounds"] and rep["chunks"] == 1
    grey = V.decode_jpeg_tensors([CASES["noise_q100_gray"], CASES["size_17x17_gray"]], channels=1)
    assert [tuple(g.shape) for g in grey] == [(64, 96), (17, 17)]
    assert np.array_equal(grey[0].cpu().numpy(), DC.reference("noise_q100_gray", 256).pixels[..., 0])
    assert V.decode_jpeg_tensors([]) == []


def test_two_batches_on_two_streams(V, singles):
    """two different batches on two streams, no device-wide synchronize in between"""
    a, b = ["noise_q100_422", "size_8x8_gray", "dri1_444"], ["midrow_420_r3", WIDE]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            ga = V.decode_jpeg_tensors([CASES[n] for n in a], subseq_bits=256)
        with torch.cuda.stream(s2):
            gb = V.decode_jpeg_tensors([CASES[n] for n in b], subseq_bits=256)
        outs.append((ga, gb))
    s1.synchronize(), s2.synchronize()
    for ga, gb in outs:
        for names, got in ((a, ga), (b, gb)):
            for n, t in zip(names, got):
                assert np.array_equal(t.cpu().numpy(), singles(n, 256)[0]), n


def test_refused_under_stream_capture(V, singles):
    """the host reads the flags between the rounds: under capture the call is refused before it does anything, as the single call is"""
    from vr180_convert_amd import _native

    lib = _native.lib()
    names = ["size_16x16_444", "size_8x8_gray"]
    n = len(names)
    outs = [torch.zeros(DC.reference(m, 256).pixels.shape, dtype=torch.uint8, device="cuda") for m in names]
    files = (C.c_char_p * n)(*[CASES[m] for m in names])
    sizes = (C.c_uint64 * n)(*[len(CASES[m]) for m in names])
    ptrs = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    pitches = (C.c_int64 * n)(*[o.stride(0) for o in outs])
    cns = (C.c_int * n)(3, 3)
    status, reports, rounds = (C.c_int * n)(7, 7), (Report * n)(), C.c_uint32(0)

    def call(stream):
        return lib.v1c_jpeg_decode_batch(0, stream.cuda_stream, n, files, sizes, ptrs, pitches, cns, 0, 0, status, reports, C.byref(rounds))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            outs[0].zero_()
            rc = call(s)
    torch.cuda.current_stream().wait_stream(s)
    assert rc == -2 and b"graph" in lib.v1c_last_error() and rounds.value == 0 and list(status) == [7, 7]  # (nothing done, nothing written)
    assert call(torch.cuda.current_stream()) == 0 and list(status) == [0, 0] and rounds.value == max(r.rounds for r in reports)
    for m, o in zip(names, outs):
        assert np.array_equal(o.cpu().numpy(), DC.reference(m, 256).pixels)


def test_per_file_status_of_refused_files_and_bad_arguments(V):
    """files the parse refuses and bad per-file arguments get the single call's return value as their status, and the batch is V1C_OK"""
    from vr180_convert_amd import _native

    lib = _native.lib()
    good = "size_17x17_420"
    files = [DC.unsupported_cases()["progressive"], DC.corrupt_cases()["no_eoi"][0], CASES[good], CASES[good], CASES[good]]
    n = len(files)
    outs = [torch.zeros((17, 17, 3), dtype=torch.uint8, device="cuda") for _ in files]
    data = (C.c_char_p * n)(*files)
    sizes = (C.c_uint64 * n)(*[len(f) for f in files])
    ptrs = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    pitches = (C.c_int64 * n)(51, 51, 50, 51, 51)
    cns = (C.c_int * n)(3, 3, 3, 1, 3)
    status, reports, rounds = (C.c_int * n)(), (Report * n)(), C.c_uint32(0)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.v1c_jpeg_decode_batch(0, st, n, data, sizes, ptrs, pitches, cns, 256, 0, status, reports, C.byref(rounds)) == 0
    assert list(status) == [-2, -5, -1, -1, 0] and reports[0].error_pos > 0 and reports[1].error_pos > 0
    assert rounds.value == reports[4].rounds >= 1 and reports[4].subsequences == DC.reference(good, 256).subsequences
    assert np.array_equal(outs[4].cpu().numpy(), DC.reference(good, 256).pixels) and not outs[2].any() and not outs[3].any()
    # all refused: nothing runs
    assert lib.v1c_jpeg_decode_batch(0, st, 2, data, sizes, ptrs, pitches, cns, 256, 0, status, reports, C.byref(rounds)) == 0
    assert list(status)[:2] == [-2, -5] and rounds.value == 0


def test_apply_lr_batch_equals_device_decode_true(V, tmp_path):
    """the docs image as both eyes: ``device_decode="batch"`` writes the bytes ``device_decode=True`` writes -- as two files (one batch
    of two) and as one side-by-side file (decoded once)"""
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder, PolynomialScaler

    chain = EquirectangularEncoder() * PolynomialScaler() * FisheyeDecoder("equidistant")
    l, r = tmp_path / "l.jpg", tmp_path / "r.jpg"
    shutil.copy(DOCS_JPG, l), shutil.copy(DOCS_JPG, r)
    kw = dict(size_output=(512, 512), interpolation=1, radius="max")
    for name, left, right in (("pair", l, r), ("sbs", l, l)):
        V.apply_lr(chain, left_path=left, right_path=right, out_path=tmp_path / f"{name}_true.png", device_decode=True, **kw)
        V.apply_lr(chain, left_path=left, right_path=right, out_path=tmp_path / f"{name}_batch.png", device_decode="batch", **kw)
        want = (tmp_path / f"{name}_true.png").read_bytes()
        assert len(want) > 10000 and (tmp_path / f"{name}_batch.png").read_bytes() == want
    rep = V.last_batch_report()
    assert rep["chunks"] == 1 and len(rep["files"]) == 1
    got = V.decode_jpeg_tensors([l, r])
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], V.decode_jpeg_tensor(DOCS_JPG))
    assert V.last_batch_report()["batch_rounds"] == V.last_decode_report()["rounds"]
