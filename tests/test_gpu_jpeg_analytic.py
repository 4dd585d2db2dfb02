"""The files the MI355X writes (``encode_jpeg_tensor``, ``encode_jpeg_tensors``) against the float64 statement of tests/jpg_analytic.py:
every quantised coefficient of every block, read back by the decoder's restatement, within q / 2 + delta + the samples' tie intervals
of the orthonormal DCT-II of the JFIF planes; the bias pair at quality 100.  No byte comparison with jpg_ref.py: that is
tests/test_gpu_jpeg.py, test_gpu_jpeg_edges.py and test_gpu_jpeg_batch.py.  tests/test_jpeg_analytic_host.py runs the same hold over the
restatement and the host build of jpeg_core.hpp, shows that wrong encoders fall outside it, and estimates the twelve DCT constants (that
takes 11 264 blocks, too many to read back from a file here; the kernels compile jpeg_core.hpp's ``fdct_pass``, which it holds)."""
import numpy as np
import pytest
import torch

import jpg_analytic as A
import jpg_cases as PC
import sphere_scene
from test_jpeg_analytic_host import QUALITIES, SUBSAMPLINGS, check, filtered, grey_noise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    import vr180_convert_amd as V
    from vr180_convert_amd import _native

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    _native.lib()
    return V


def _dev(img):
    return torch.from_numpy(np.ascontiguousarray(img)).cuda()


def _hold(V, label, img, quality, subsampling, view=None, **kw):
    """one single call, held; ``view``: the device tensor to encode where it is not a dense copy of ``img``"""
    data = V.encode_jpeg_tensor(_dev(img) if view is None else view, quality=quality, subsampling=subsampling, **kw)
    f = A.hold_file(data, img, quality, subsampling)
    check(f"gpu {label} {subsampling} q{quality}", f)
    return data, f


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("subsampling", SUBSAMPLINGS)
def test_single_calls_hold(V, subsampling, quality):
    worst = -1.0
    for i, (h, w) in enumerate(PC.SIZES):
        for cn in (1, 3, 4):
            if cn == 1 and subsampling != "420":
                continue  # (a grey file does not depend on the option)
            img = (PC.noise if i % 2 else PC.smooth)(h, w, cn, 100 + 10 * i + cn)
            worst = max(worst, _hold(V, f"size {h}x{w} cn{cn}", img, quality, subsampling)[1]["max"])
    for kind in ("noise", "smooth"):
        f = _hold(V, f"cells {kind}", filtered(kind), quality, subsampling)[1]
        assert f["ambiguous"] == 0
        worst = max(worst, f["max"])
    if quality == 100 and subsampling == "420":
        worst = max(worst, _hold(V, "swing", PC.swing()[..., None], 100, "420")[1]["max"])
    print(f"gpu single {subsampling} q{quality}: largest |c q - F| - q / 2 - interval term = {worst:.4f} (delta {A.DELTA:.4f})")


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("subsampling", SUBSAMPLINGS)
def test_pitched_views_behind_odd_offsets_hold(V, subsampling, quality):
    whole = PC.smooth(48, 128, 3, 90)
    t = _dev(whole)
    window, right = t[:, 31:76], t[:, 64:]
    assert not window.is_contiguous() and window.data_ptr() % 2 == 1 and not right.is_contiguous()
    _hold(V, "columns 31 ... 75 of 48 x 128", whole[:, 31:76], quality, subsampling, view=window)
    _hold(V, "right half of a side-by-side tensor", whole[:, 64:], quality, subsampling, view=right)


@pytest.mark.parametrize("subsampling", SUBSAMPLINGS)
def test_restart_interval_moves_no_coefficient(V, subsampling):
    """5 x 3 MCUs of 16 or 9 x 5 of 8: one MCU per interval, the default (a row), and 7, which ends mid-row"""
    img = PC.smooth(40, 72, 3, 50)
    files = [_hold(V, f"restart {r}", img, 95, subsampling, restart_mcus=r)[0] for r in (None, 1, 7)]
    coefs = [A.file_coefficients(d)[0] for d in files]
    assert len(set(files)) == 3  # (the files do differ: DRI, the markers, the DC differences)
    assert np.array_equal(coefs[0], coefs[1]) and np.array_equal(coefs[0], coefs[2])


def test_one_batch_of_mixed_images_holds_and_equals_the_single_calls(V):
    sbs = _dev(PC.smooth(48, 128, 3, 90))
    half = sbs[:, 64:]
    assert not half.is_contiguous()
    members = [  # (image on the host, the tensor to encode, quality, subsampling)
        (PC.noise(1, 1, 1, 301), None, 95, "420"), (PC.noise(1, 1, 3, 302), None, 100, "444"), (PC.smooth(7, 9, 3, 303), None, 50, "420"),
        (PC.noise(17, 17, 4, 304), None, 1, "420"), (PC.smooth(15, 33, 1, 305), None, 100, "444"), (PC.noise(31, 16, 4, 306), None, 95, "444"),
        (filtered("noise"), None, 100, "420"), (filtered("smooth"), None, 95, "444"), (sbs.cpu().numpy()[:, 64:], half, 80, "420"),
        (np.ascontiguousarray(sphere_scene.render(301)[100:196, 100:196]), None, 95, "420"), (grey_noise(), None, 100, "420"),
    ]
    tensors = [_dev(img) if t is None else t for img, t, _, _ in members]
    files = V.encode_jpeg_tensors(tensors, quality=[m[2] for m in members], subsampling=[m[3] for m in members])
    assert V.last_encode_batch_report()["chunks"] == 1 and len(files) == len(members)
    for k, ((img, _, q, sub), t, data) in enumerate(zip(members, tensors, files)):
        check(f"gpu batch member {k} {img.shape} {sub} q{q}", A.hold_file(data, img, q, sub))
        assert data == V.encode_jpeg_tensor(t, quality=q, subsampling=sub), k


@pytest.mark.parametrize("subsampling", SUBSAMPLINGS)
def test_bias_at_quality_100_through_both_entry_points(V, subsampling):
    imgs = [("cells_noise", filtered("noise")), ("grey_noise", grey_noise())]
    batch = V.encode_jpeg_tensors([_dev(img) for _, img in imgs], quality=100, subsampling=subsampling)
    for (label, img), data in zip(imgs, batch):
        single = V.encode_jpeg_tensor(_dev(img), quality=100, subsampling=subsampling)
        check(f"gpu bias single {label} {subsampling}", A.hold_file(single, img, 100, subsampling), bias=True)
        check(f"gpu bias batch {label} {subsampling}", A.hold_file(data, img, 100, subsampling), bias=True)
