"""The device PNG encoder on the MI355X at the boundaries of its kernels (tests/png_cases.py): run planes laid across the 64-lane
steps and the segment start of ``load_segment``, bands of a whole number of segments and with a 1-byte last segment, 64 / 65 and 256 /
257 segments (the group split, the scan's carry), 15-bit codes and package-merged trees, stored bands around the 65 535-byte block,
BGR / BGRA / 16-bit forms of the same planes -- both filters, contiguous, as the right half of a wider tensor and behind an odd byte
offset, against the NumPy restatement (png_ref.py): segments, every band record, the file.  tests/test_png_device_host.py runs the
same images through the host build of the arithmetic and the planner, which tells a wrong rule from wrong kernel plumbing."""
import numpy as np
import pytest
import torch

import png_cases as PC
import png_ref as R

pytestmark = pytest.mark.gpu
PARAMS = [(name, f) for name in PC.shared_cases() for f in ("up", "paeth")]


@pytest.fixture(scope="module")
def P():
    from vr180_convert_amd import _native, png_device

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    _native.lib()
    return png_device


def views(img):
    """(label, device view) of the image: contiguous, the right half of a wider tensor, and -- 8-bit -- behind an odd byte offset"""
    h, w, cn = img.shape
    rng = np.random.default_rng(h * 1000 + w)
    yield "contiguous", torch.from_numpy(img).cuda()
    left = rng.integers(0, 256, (h, w + 3, cn)).astype(img.dtype)
    sbs = torch.from_numpy(np.concatenate([left, img], axis=1)).cuda()
    yield "right half", sbs[:, w + 3:]
    if img.dtype == np.uint8:
        row = w * cn
        flat = rng.integers(0, 256, 5 + h * (row + 6), dtype=np.uint8)
        np.lib.stride_tricks.as_strided(flat[5:], (h, row), (row + 6, 1))[...] = img.reshape(h, row)
        yield "odd offset", torch.as_strided(torch.from_numpy(flat).cuda(), (h, w, cn), (row + 6, cn, 1), 5)


@pytest.mark.parametrize("name,filter", PARAMS)
def test_edge_image_equals_restatement(P, name, filter):
    img, rows = PC.shared_cases()[name]
    wsegs, wbands, wfile = PC.reference(name, filter)
    R.check_file(wfile, img, filter, rows)
    for label, t in views(img):
        assert label == "contiguous" or not t.is_contiguous() or img.shape[0] == 1
        segs, bands = P.deflate_tensor(t, filter=filter, band_rows=rows)
        segs = segs.tobytes()  # (copied out before the next call on this device reuses the buffer)
        assert bands == wbands, (label, [k for k, (a, b) in enumerate(zip(bands, wbands)) if a != b][:8])
        assert segs == wsegs, (label, len(segs), len(wsegs), next((i for i, (a, b) in enumerate(zip(segs, wsegs)) if a != b), None))
        got = P.encode_png_tensor(t, filter=filter, band_rows=rows)
        assert got == wfile, label
        assert P.encode_png_tensor(t, filter=filter, band_rows=rows) == got, label  # two calls: identical bytes


def test_two_streams_back_to_back(P):
    """two different images on two streams, no device-wide synchronize in between; each result is copied out (bytes) before the next
    call on the device, as deflate_tensor's docstring asks"""
    cases = PC.shared_cases()
    (a, ra), (b, rb) = cases["runs_65792"], cases["noise_then_runs"]
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    out = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            out.append(P.encode_png_tensor(ta, filter="paeth", band_rows=ra))
        with torch.cuda.stream(s2):
            out.append(P.encode_png_tensor(tb, filter="up", band_rows=rb))
    torch.cuda.synchronize()
    assert out[0::2] == [PC.reference("runs_65792", "paeth")[2]] * 3
    assert out[1::2] == [PC.reference("noise_then_runs", "up")[2]] * 3
