"""The device JPEG encoder on the MI355X at the boundaries of its kernels (tests/jpg_cases.py): partial MCUs in either axis for both
subsamplings, intervals that end mid-row, of one MCU, of all MCUs and of more, RSTm wrapping, EOB-only blocks, blocks without EOB,
ZRL runs, the largest categories, stuffed bytes, intervals without a pad and with a 0xFF pad byte, five qualities, grey / BGR / BGRA,
contiguous images, the right half of a wider tensor and views behind an odd byte offset -- through ``v1c_jpeg_encode`` against the
NumPy restatement (jpg_ref.py), byte for byte.  tests/test_jpeg_device_host.py runs the same images through the host build of the
arithmetic, which tells a wrong rule from wrong kernel plumbing."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpg_cases as PC
import jpg_ref as R

pytestmark = pytest.mark.gpu
CASES = PC.shared_cases()


@pytest.fixture(scope="module")
def lib():
    from vr180_convert_amd import _native

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    return _native.lib()


def scan_of(lib, c, base, stream=None):
    """the scan of a case whose buffer lies on the device as ``base``, through the C ABI"""
    sub = R.SUBSAMPLINGS[c.subsampling]
    cap = int(lib.v1c_jpeg_bound(c.h, c.w, c.cn, sub, c.restart))
    out = np.zeros(cap, np.uint8)
    size = C.c_uint64(0)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    rc = lib.v1c_jpeg_encode(0, st, base.data_ptr() + c.offset, c.h, c.w, c.pitch, c.cn, c.quality, sub, c.restart, out.ctypes.data, cap,
                             C.byref(size))
    assert rc == 0, lib.v1c_last_error()
    return out[:size.value].tobytes()


def want_scan(name):
    c = CASES[name]
    data = PC.reference(name)[2]
    head = R.headers(R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart), c.quality)
    assert data.startswith(head)
    return data[len(head):-2]


@pytest.mark.parametrize("name", list(CASES))
def test_edge_image_equals_restatement(lib, name):
    c = CASES[name]
    base = torch.from_numpy(c.base).cuda()
    got, want = scan_of(lib, c, base), want_scan(name)
    assert got == want, (len(got), len(want), next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None))
    assert scan_of(lib, c, base) == got  # two calls: identical bytes


def test_two_streams_back_to_back(lib):
    """two different images on two streams, no device-wide synchronize in between"""
    na, nb = "noise_q100_420", "restart1_444"
    ta, tb = torch.from_numpy(CASES[na].base).cuda(), torch.from_numpy(CASES[nb].base).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    out = []
    for _ in range(3):
        out.append(scan_of(lib, CASES[na], ta, s1))
        out.append(scan_of(lib, CASES[nb], tb, s2))
    torch.cuda.synchronize()
    assert out[0::2] == [want_scan(na)] * 3
    assert out[1::2] == [want_scan(nb)] * 3
