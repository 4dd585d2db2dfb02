"""The device PNG encoder on the MI355X: ``encode_png_tensor`` against the NumPy restatement (png_ref.py) byte for byte, the readers
the contract names, a real remap result, and the ``device_png`` route of ``apply`` / ``apply_lr`` against the host route."""
import io
from pathlib import Path

import numpy as np
import pytest
import torch

import png_ref as R
import sphere_scene as S

pytestmark = pytest.mark.gpu
CASES = R.cases()
PARAMS = [(name, f) for name in CASES for f in ("up", "paeth")]


@pytest.fixture(scope="module")
def P():
    from vr180_convert_amd import _native, png_device

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    _native.lib()
    return png_device


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pil_bgr(png):
    from PIL import Image

    with Image.open(io.BytesIO(png)) as im:
        a = np.asarray(im)
    return a if a.ndim == 2 else a[..., ::-1] if a.shape[2] == 3 else a[..., [2, 1, 0, 3]]


@pytest.mark.parametrize("name,filter", PARAMS)
def test_equals_restatement_byte_for_byte(P, name, filter):
    img, rows = CASES[name]
    got = P.encode_png_tensor(_dev(img), filter=filter, band_rows=rows)
    assert got == R.encode(img, filter=filter, band_rows=rows)
    R.check_file(got, img, filter, rows)
    assert P.encode_png_tensor(_dev(img), filter=filter, band_rows=rows) == got  # two calls: identical bytes


def test_two_dimensional_gray_and_default_bands(P):
    img = S.render(1024)
    stride = 1 + 1024 * 3
    rows = P.default_band_rows(1024, stride)
    assert rows == 64
    got = P.encode_png_tensor(_dev(img))
    assert got == R.encode(img, band_rows=rows)
    gray = np.ascontiguousarray(img[..., 0])
    got = P.encode_png_tensor(_dev(gray), band_rows=8)
    assert got == R.encode(gray[..., None], band_rows=8)
    assert np.array_equal(_pil_bgr(got), gray)


def test_pitched_half_of_a_side_by_side_tensor(P):
    left, right = S.render(512), S.render(512, S.rotation([0.3, 1, 0.2], 4))
    sbs = _dev(np.concatenate([left, right], axis=1))
    for half, want in ((sbs[:, :512], left), (sbs[:, 512:], right)):
        assert not half.is_contiguous()
        assert P.encode_png_tensor(half, band_rows=8) == R.encode(want, band_rows=8)
    sbs16 = _dev(np.concatenate([left, right], axis=1).astype(np.uint16) * 257)
    assert P.encode_png_tensor(sbs16[:, 512:], filter="paeth", band_rows=16) == R.encode(right.astype(np.uint16) * 257, filter="paeth",
                                                                                          band_rows=16)


def test_non_default_stream(P):
    from vr180_convert_amd.synth import pattern

    img = pattern(700, 900)
    want = R.encode(img, band_rows=8)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = _dev(img)
        got = P.encode_png_tensor(t, band_rows=8)
    st.synchronize()
    assert got == want


def test_full_size_side_by_side_frame(P):
    """8192 x 4096 x 3: the shape the band count and the scans are sized for (512 bands of 8 rows; noise bands stored, drawn bands coded)"""
    from vr180_convert_amd import _png
    from vr180_convert_amd.synth import noise_disc, pattern

    img = np.concatenate([pattern(4096, 4096), noise_disc(4096, 4096, 1)], axis=1)
    t = _dev(img)
    got = P.encode_png_tensor(t)
    assert P.encode_png_tensor(t) == got
    segs, bands = P.deflate_tensor(t)
    assert len(bands) == 512
    own = _png.decode(got)
    assert own is not None and np.array_equal(own, img)
    assert got == R.encode(img, band_rows=8)


def test_a_real_result(P):
    import vr180_convert_amd as V
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder

    left, right = S.render(2048), S.render(2048, S.rotation([0.3, 1, 0.2], 4))
    t = EquirectangularEncoder() * FisheyeDecoder("equidistant")
    sbs = V.apply_lr_tensors(t, _dev(left), _dev(right), size_output=(2048, 2048), interpolation=1, radius="max")
    png = V.encode_png_tensor(sbs)
    assert np.array_equal(_pil_bgr(png), sbs.cpu().numpy())


def _read(path):
    from PIL import Image

    if str(path).endswith(".npy"):
        return np.load(path)
    with Image.open(path) as im:
        return np.asarray(im)


def test_apply_lr_device_png_equals_the_host_route(P, tmp_path, monkeypatch):
    import vr180_convert_amd as V
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder

    calls = []
    orig = P.imwrite_tensor
    monkeypatch.setattr(P, "imwrite_tensor", lambda p, t, **k: (calls.append(Path(p).name), orig(p, t, **k))[1])
    left, right = S.render(512), S.render(512, S.rotation([0.3, 1, 0.2], 4))
    t = EquirectangularEncoder() * FisheyeDecoder("equidistant")
    kw = dict(left_path=left, right_path=right, size_output=(512, 512), interpolation=1, radius="max")
    V.apply_lr(t, out_path=tmp_path / "d.png", device_png=True, **kw)
    V.apply_lr(t, out_path=tmp_path / "h.png", device_png=False, **kw)
    assert calls == ["d.png"]
    assert np.array_equal(_read(tmp_path / "d.png"), _read(tmp_path / "h.png")) and _read(tmp_path / "d.png").shape == (512, 1024, 3)
    # 16-bit eyes: a 16-bit PNG either way
    l16, r16 = left.astype(np.uint16) * 257, right.astype(np.uint16) * 257
    kw16 = dict(kw, left_path=l16, right_path=r16)
    V.apply_lr(t, out_path=tmp_path / "d16.png", device_png=True, **kw16)
    V.apply_lr(t, out_path=tmp_path / "h16.png", device_png=False, **kw16)
    assert calls == ["d.png", "d16.png"]
    a, b = R.decode((tmp_path / "d16.png").read_bytes()), R.decode((tmp_path / "h16.png").read_bytes())
    assert a.dtype == np.uint16 and np.array_equal(a, b)
    # merge=True and other formats take the host route
    V.apply_lr(t, out_path=tmp_path / "m.png", device_png=True, merge=True, **kw)
    V.apply_lr(t, out_path=tmp_path / "n.npy", device_png=True, **kw)
    V.apply_lr(t, out_path=tmp_path / "j.jpg", device_png=True, **kw)
    assert calls == ["d.png", "d16.png"]
    assert (tmp_path / "m.png").exists() and np.array_equal(_read(tmp_path / "n.npy")[..., ::-1], _read(tmp_path / "d.png"))


def test_apply_device_png_equals_the_host_route(P, tmp_path, monkeypatch):
    import vr180_convert_amd as V
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder

    calls = []
    orig = P.imwrite_tensor
    monkeypatch.setattr(P, "imwrite_tensor", lambda p, t, **k: (calls.append(Path(p).name), orig(p, t, **k))[1])
    imgs = [_dev(S.render(384)), _dev(S.render(384, S.rotation([0.3, 1, 0.2], 4))), _dev(S.render(384, S.rotation([1, 0, 0], 7)))]
    t = EquirectangularEncoder() * FisheyeDecoder("equidistant")
    kw = dict(in_paths=imgs, size_output=(384, 384), interpolation=1, radius="max")
    V.apply(t, out_paths=[tmp_path / "a.png", tmp_path / "b.npy", tmp_path / "c.png"], device_png=True, **kw)
    V.apply(t, out_paths=[tmp_path / "ha.png", tmp_path / "hb.npy", tmp_path / "hc.png"], **kw)
    assert calls == ["a.png", "c.png"]
    for n in ("a.png", "b.npy", "c.png"):
        assert np.array_equal(_read(tmp_path / n), _read(tmp_path / ("h" + n))), n
