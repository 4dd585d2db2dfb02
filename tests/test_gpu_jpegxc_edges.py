"""The lossless JPEG transcoder on the MI355X at the boundaries of its kernels (tests/jpgxc_cases.py): images of one, 2 x 2 and 3 x 2
MCUs in grey, 4:4:4, 4:2:2 and 4:2:0; crops of the first, the last and the partial last column and row; swaps whose halves are one MCU wide;
outputs of 31 ... 33, 255 ... 257 and 511 ... 513 blocks; sources with restart markers every 1, 2 and 7 MCUs cut inside an interval,
outputs with every MCU an interval, a row and none; a source whose decode takes many rounds; optimised tables on a flat image and on
noise -- through ``v1c_jpeg_transcode`` at 256-bit subsequences and at the default against the restatement (jpgxc_ref.py), byte for
byte, header and scan.  tests/test_jpegxc_host.py runs the same cases through the host build of the arithmetic, which tells a wrong rule
from wrong kernel plumbing."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpgdec_cases as JC
import jpgdec_ref as D
import jpgxc_cases as K
import jpgxc_ref as X
from test_jpegxc_host import _xc_outputs

pytestmark = pytest.mark.gpu
CASES = K.cases()


class Report(C.Structure):
    _fields_ = [("segments", C.c_uint32), ("subsequences", C.c_uint32), ("rounds", C.c_uint32), ("reserved", C.c_uint32),
                ("error_pos", C.c_uint64)]


@pytest.fixture(scope="module")
def lib():
    from vr180_convert_amd import _native

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    return _native.lib()


def transcode(lib, data, outputs, S=0, stream=None):
    """through the C ABI: (return code, report, every output's file)"""
    src = None
    try:
        src = X.Source(data)
    except Exception:  # noqa: BLE001 - a file the restatement refuses: the default restart interval does not matter
        pass
    outs, keep = _xc_outputs(outputs, src)
    bounds = [max(int(lib.v1c_jpeg_transcode_bound(data, len(data), o.width, o.height, o.restart_mcus)), 1 << 12) for o in outs]
    buf = np.full(sum(bounds), 0xA5, np.uint8)
    at = 0
    for o, b in zip(outs, bounds):
        o.out_host, o.capacity = buf.ctypes.data + at, b
        at += b
    rep = Report()
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    rc = lib.v1c_jpeg_transcode(0, st, data, len(data), len(outputs), outs, S, C.byref(rep))
    files, at = [], 0
    for o, b in zip(outs, bounds):
        if rc == 0:
            head = (C.c_uint8 * 2048)()
            n = lib.v1c_jpeg_header_xc(data, len(data), o.width, o.height, o.restart_mcus, o.dht if o.optimize else None, o.dht_size, head, 2048)
            assert n > 0, lib.v1c_last_error()
            files.append(bytes(head[:n]) + buf[at:at + int(o.size)].tobytes() + b"\xff\xd9")
            assert (buf[at + int(o.size):at + b] == 0xA5).all()  # nothing behind the scan is written
        at += b
    return rc, rep, files


@pytest.mark.parametrize("name", list(CASES))
def test_edge_case_equals_restatement(lib, name):
    data, outputs = CASES[name]
    want = list(K.reference(name))
    for S in (256, 0):
        rc, rep, files = transcode(lib, data, outputs, S)
        assert rc == 0, lib.v1c_last_error()
        assert files == want, (S, [len(f) for f in files], [len(f) for f in want])
        assert rep.segments == D.parse(data).nseg and rep.rounds >= 1
    rc, _, again = transcode(lib, data, outputs, 0)
    assert rc == 0 and again == want  # two calls: identical bytes


def test_many_rounds_case_takes_them(lib):
    data, outputs = CASES[K.SLOW_ROUNDS]
    rc, rep, files = transcode(lib, data, outputs, 256)
    assert rc == 0 and files == list(K.reference(K.SLOW_ROUNDS))
    assert 5 < rep.rounds <= D.decode(data, 256, check=False).rounds


def test_two_streams_back_to_back(lib):
    """two different files on two streams, no device-wide synchronize in between"""
    na, nb = "noise_q100_444_swap", "source_dri7_420"
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    got = []
    for _ in range(3):
        got.append(transcode(lib, *CASES[na], 256, stream=s1))
        got.append(transcode(lib, *CASES[nb], 256, stream=s2))
    s1.synchronize(), s2.synchronize()
    assert all(rc == 0 and f == list(K.reference(na)) for rc, _, f in got[0::2])
    assert all(rc == 0 and f == list(K.reference(nb)) for rc, _, f in got[1::2])


def test_truncated_scan_is_reported_and_the_next_call_is_right(lib):
    data, outputs, by_parse = K.corrupt()[JC.TRUNCATED]
    assert not by_parse
    rc, rep, _ = transcode(lib, data, outputs, 256)
    assert rc == -5 and b"damaged" in lib.v1c_last_error()
    with pytest.raises(D.Corrupt, match=f"bit {rep.error_pos} "):
        D.decode(data, 256, check=False)
    name = "quadrants_420"
    rc, _, files = transcode(lib, *CASES[name], 256)
    assert rc == 0 and files == list(K.reference(name))


def test_coefficients_outside_the_encoder_s_range_are_refused(lib):
    """valid syntax, numbers beyond 8-bit samples: the gather raises its flag and the encoder's chain is never launched; the call behind
    it is right"""
    for name, (data, outputs) in K.out_of_range().items():
        rc, _, _ = transcode(lib, data, outputs)
        assert rc == -2 and b"coefficient" in lib.v1c_last_error(), name
    for name, (data, outputs) in K.excluded_blocks().items():  # the same kind of block, left out by the cut: taken
        rc, _, files = transcode(lib, data, outputs)
        assert rc == 0 and files == X.transcode(data, outputs), name
    rc, _, files = transcode(lib, *CASES["coefficient_limits"])
    assert rc == 0 and files == list(K.reference("coefficient_limits"))


def test_refused_under_stream_capture(lib):
    """the host reads flags and sizes between the kernels: under capture the call is refused before it does anything"""
    name = "whole_2x2_444"
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    scratch = torch.zeros(16, device="cuda")
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            scratch.zero_()
            rc, _, _ = transcode(lib, *CASES[name], 0, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    assert rc == -2 and b"graph" in lib.v1c_last_error()
    rc, _, files = transcode(lib, *CASES[name], 0)
    assert rc == 0 and files == list(K.reference(name))
