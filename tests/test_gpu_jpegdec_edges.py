"""The device JPEG decoder on the MI355X at the boundaries of its kernels (tests/jpgdec_cases.py): partial MCUs in either axis for
grey, 4:4:4, 4:2:2 and 4:2:0, every kind of restart interval and none, subsequences entered mid-block, mid-MCU and off the grid,
EOB-only blocks, blocks without EOB, ZRL runs, the largest categories, stuffed bytes on piece boundaries, optimised tables, 16-bit
DQT, fill bytes, merged DHT -- through ``v1c_jpeg_decode`` at 256-bit subsequences and at the default against the restatement
(jpgdec_ref.py), byte for byte.  tests/test_jpegdec_host.py runs the same files through the host build of the arithmetic, which tells
a wrong rule from wrong kernel plumbing."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpgdec_cases as DC

pytestmark = pytest.mark.gpu
CASES = {**DC.supported_cases(), **DC.extreme_cases()}


class Report(C.Structure):
    _fields_ = [("segments", C.c_uint32), ("subsequences", C.c_uint32), ("rounds", C.c_uint32), ("reserved", C.c_uint32),
                ("error_pos", C.c_uint64)]


@pytest.fixture(scope="module")
def lib():
    from vr180_convert_amd import _native

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    return _native.lib()


def decode(lib, data, S, out, cn=3, stream=None):
    """through the C ABI into the (h, w[, cn]) device tensor ``out`` (rows may be pitched): (return code, report)"""
    rep = Report()
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    rc = lib.v1c_jpeg_decode(0, st, data, len(data), out.data_ptr(), out.stride(0), cn, S, C.byref(rep))
    return rc, rep


@pytest.mark.parametrize("name", list(CASES))
def test_edge_file_equals_restatement(lib, name):
    for S in (256, 0):
        want = DC.reference(name, S)
        h, w = want.pixels.shape[:2]
        out = torch.full((h, w, 3), 0xA5, dtype=torch.uint8, device="cuda")
        rc, rep = decode(lib, CASES[name], S, out)
        assert rc == 0, lib.v1c_last_error()
        got = out.cpu().numpy()
        assert np.array_equal(got, want.pixels), (S, int((got != want.pixels).sum()))
        assert (rep.segments, rep.subsequences) == (want.segments, want.subsequences)
        assert 1 <= rep.rounds <= want.rounds
        again = torch.zeros_like(out)
        assert decode(lib, CASES[name], S, again)[0] == 0
        assert torch.equal(again, out)  # two calls: identical bytes


def test_left_half_of_a_wider_tensor(lib):
    name = "noise_q100_420"
    want = DC.reference(name, 256).pixels
    h, w = want.shape[:2]
    whole = torch.full((h, 2 * w + 3, 3), 0x5A, dtype=torch.uint8, device="cuda")
    rc, _ = decode(lib, CASES[name], 256, whole[:, :w])
    assert rc == 0, lib.v1c_last_error()
    got = whole.cpu().numpy()
    assert np.array_equal(got[:, :w], want) and (got[:, w:] == 0x5A).all()
    # ... and behind an odd byte offset, where no row is aligned
    rc, _ = decode(lib, CASES[name], 256, whole[:, w + 1:2 * w + 1])
    assert rc == 0
    got = whole.cpu().numpy()
    assert np.array_equal(got[:, w + 1:2 * w + 1], want) and (got[:, w] == 0x5A).all() and (got[:, 2 * w + 1:] == 0x5A).all()


@pytest.mark.parametrize("name", ["size_17x17_gray", "noise_q100_gray", "dri1_gray"])
def test_one_channel_for_grey(lib, name):
    want = DC.reference(name).pixels
    h, w = want.shape[:2]
    out = torch.zeros((h, w + 5), dtype=torch.uint8, device="cuda")
    rc, _ = decode(lib, CASES[name], 0, out[:, :w], cn=1)
    assert rc == 0, lib.v1c_last_error()
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :w], want[..., 0]) and not got[:, w:].any()


def test_two_streams_back_to_back(lib):
    """two different files on two streams, no device-wide synchronize in between"""
    na, nb = "noise_q100_422", "dri1_444"
    wa, wb = DC.reference(na, 256).pixels, DC.reference(nb, 256).pixels
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


def test_truncated_scan_is_reported_and_the_next_decode_is_right(lib):
    """(the stand-alone sanitizer run of tests/test_jpegdec_host.py shows that truncated input keeps every read in bounds)"""
    data = DC.corrupt_cases()[DC.TRUNCATED][0]
    out = torch.zeros((24, 40, 3), dtype=torch.uint8, device="cuda")
    rc, rep = decode(lib, data, 256, out)
    assert rc == -5 and b"damaged" in lib.v1c_last_error()
    name = "size_15x33_420"
    want = DC.reference(name, 256).pixels
    out = torch.zeros(want.shape, dtype=torch.uint8, device="cuda")
    assert decode(lib, CASES[name], 256, out)[0] == 0
    assert np.array_equal(out.cpu().numpy(), want)


def test_refused_under_stream_capture(lib):
    """the host reads a flag between the rounds: under capture the call is refused before it does anything"""
    name = "size_16x16_444"
    out = torch.zeros((16, 16, 3), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out.zero_()
            rc, _ = decode(lib, CASES[name], 0, out, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    assert rc == -2 and b"graph" in lib.v1c_last_error()
    assert decode(lib, CASES[name], 0, out)[0] == 0
    assert np.array_equal(out.cpu().numpy(), DC.reference(name).pixels)
