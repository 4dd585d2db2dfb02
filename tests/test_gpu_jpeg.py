"""The device JPEG encoder on the MI355X through its Python interface: natural images, a 2048 x 2048 pair result and one 8192 x 4096
frame against the NumPy restatement (jpg_ref.py), the file byte for byte; ``apply`` / ``apply_lr`` with ``device_jpeg=True``; results
that are not eligible; repeated calls."""
import io

import numpy as np
import pytest
import torch

import jpg_ref as R
import sphere_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    import vr180_convert_amd as V
    from vr180_convert_amd import _native

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    _native.lib()
    return V


def _chain():
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder, PolynomialScaler

    return EquirectangularEncoder() * PolynomialScaler([0, 1, -0.1]) * FisheyeDecoder("equidistant")


def _pil(data):
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    im.load()
    return im


@pytest.mark.parametrize("subsampling,quality", [("420", 95), ("444", 95), ("420", 50), ("444", 30)])
def test_natural_images_equal_restatement(V, tmp_path, subsampling, quality):
    from vr180_convert_amd import synth

    for img in (sphere_scene.render(301)[:240], synth.pattern(200, 136), synth.noise_disc(96, 96)[..., 1]):
        t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
        got = V.encode_jpeg_tensor(t, quality=quality, subsampling=subsampling)
        assert got == R.encode(img, quality, subsampling)
        assert _pil(got).size == (img.shape[1], img.shape[0])
        V.imwrite_jpeg_tensor(tmp_path / "a.jpg", t, quality=quality, subsampling=subsampling, restart_mcus=7)
        assert (tmp_path / "a.jpg").read_bytes() == R.encode(img, quality, subsampling, 7)
        assert V.encode_jpeg_tensor(t, quality=quality, subsampling=subsampling) == got  # repeated calls: identical bytes


def test_pair_result_2048(V):
    """a 2048 x 2048 pair: the side-by-side result as it lies on the device, and its right eye encoded in place (pitched rows)"""
    from vr180_convert_amd.synth import noise_disc

    dev = torch.device("cuda", 0)
    left, right = sphere_scene.render(1024), noise_disc(1024, 1024, 1)
    sbs = V.apply_lr_tensors(_chain(), torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev), size_output=(2048, 2048),
                             interpolation=1, radius="max")
    host = sbs.cpu().numpy()
    assert host.shape == (2048, 4096, 3)
    assert V.encode_jpeg_tensor(sbs) == R.encode(host)
    eye = sbs[1000:1500, 2048:]
    assert not eye.is_contiguous()
    assert V.encode_jpeg_tensor(eye, subsampling="444", quality=90) == R.encode(host[1000:1500, 2048:], 90, "444")


def _intervals(scan):
    """the intervals of a scan: cut at the RSTm markers (a 0xFF data byte is always followed by 0x00)"""
    a = np.frombuffer(scan, np.uint8)
    at = np.nonzero((a[:-1] == 0xFF) & (a[1:] >= 0xD0) & (a[1:] <= 0xD7))[0]
    assert [int(a[i + 1]) - 0xD0 for i in at] == [k % 8 for k in range(len(at))]
    edges = np.concatenate([[0], at + 2, [len(a) + 2]])
    return [scan[edges[k]:edges[k + 1] - 2] for k in range(len(edges) - 1)]


def test_frame_8192x4096(V):
    """One whole frame.  The restatement of 33 Mpixel takes too long for a test, so: the default interval is one MCU row, an interval
    depends on nothing outside it, and the restatement of a 16-row strip is that interval -- pinned byte for byte on rows of every kind
    of content, the first and the last; and Pillow decodes the whole file to the pixels it decodes from the restatement of a
    64-row band (but for the band's outermost rows, whose chroma Pillow interpolates across the cut)."""
    y, x = np.mgrid[0:1024, 0:2048].astype(np.float32)
    rng = np.random.default_rng(7)
    tile = np.stack([128 + 100 * np.sin(x * 0.003 * (k + 1) + y * 0.002) + rng.normal(0, 4, x.shape).astype(np.float32) for k in range(3)], axis=-1)
    img = np.tile(np.clip(tile, 0, 255).astype(np.uint8), (4, 4, 1))
    img[1000:1400, 3000:5000] = rng.integers(0, 256, (400, 2000, 3), dtype=np.uint8)
    assert img.shape == (4096, 8192, 3)
    got = V.encode_jpeg_tensor(torch.from_numpy(img).cuda())
    g = R.Geom(4096, 8192, 3)
    head = R.headers(g, 95)
    assert g.restart == 512 and g.nint == 256 and got.startswith(head) and got.endswith(b"\xff\xd9")
    parts = _intervals(got[len(head):-2])
    assert len(parts) == 256
    for r in (0, 1, 61, 62, 63, 75, 87, 88, 128, 254, 255):
        strip = img[16 * r:16 * r + 16]
        want = R.scan(R.coefficients(strip), R.Geom(16, 8192, 3))
        assert parts[r] == want, r
    im = _pil(got)
    assert im.size == (8192, 4096) and im.mode == "RGB"
    full = np.asarray(im)[960:1024]
    band = np.asarray(_pil(R.encode(img[960:1024])))
    assert np.array_equal(full[2:-2], band[2:-2])


def test_apply_lr_and_apply_write_through_the_device_encoder(V, tmp_path, monkeypatch):
    from vr180_convert_amd import _io, jpeg_device
    from vr180_convert_amd.synth import noise_disc

    dev = torch.device("cuda", 0)
    left, right = noise_disc(256, 256, 0), sphere_scene.render(256)
    host_writes, dev_writes = [], []
    real_host, real_dev = _io.imwrite, jpeg_device.imwrite_jpeg_tensor
    monkeypatch.setattr(_io, "imwrite", lambda p, a, *k, **kw: host_writes.append(str(p)) or real_host(p, a, *k, **kw))
    monkeypatch.setattr(jpeg_device, "imwrite_jpeg_tensor", lambda p, t, **kw: dev_writes.append(str(p)) or real_dev(p, t, **kw))
    sbs = V.apply_lr_tensors(_chain(), torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev), size_output=(256, 256),
                             interpolation=1, radius="max").cpu().numpy()
    out = tmp_path / "sbs.jpg"
    V.apply_lr(_chain(), left_path=left, right_path=right, out_path=out, size_output=(256, 256), interpolation=1, radius="max",
               device_jpeg=True)
    assert dev_writes == [str(out)] and host_writes == []
    want = R.encode(sbs)
    assert out.read_bytes() == want
    assert np.array_equal(np.asarray(_pil(out.read_bytes())), np.asarray(_pil(want)))
    # apply: device tensors in, so the results are still on the device when they are written
    outs = [tmp_path / "l.jpeg", tmp_path / "r.png"]
    res = V.apply(_chain(), in_paths=[torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)], out_paths=outs, size_output=(256, 256),
                  interpolation=1, radius="max", device_jpeg=True)
    assert dev_writes == [str(out), str(outs[0])]
    assert outs[0].read_bytes() == R.encode(res[0].cpu().numpy())
    assert np.array_equal(_io.imread(outs[1]), res[1].cpu().numpy())
    # not eligible: merge=True, a 16-bit result, another suffix, and the option left off -- all through the host writer
    dev_writes.clear(), host_writes.clear()
    V.apply_lr(_chain(), left_path=left, right_path=right, out_path=tmp_path / "m.jpg", size_output=(256, 256), interpolation=1, radius="max",
               merge=True, device_jpeg=True)
    V.apply_lr(_chain(), left_path=left.astype(np.uint16) * 257, right_path=right.astype(np.uint16) * 257, out_path=tmp_path / "w.jpg",
               size_output=(256, 256), interpolation=1, radius="max", device_jpeg=True)
    V.apply_lr(_chain(), left_path=left, right_path=right, out_path=tmp_path / "p.png", size_output=(256, 256), interpolation=1, radius="max",
               device_jpeg=True)
    V.apply_lr(_chain(), left_path=left, right_path=right, out_path=tmp_path / "h.jpg", size_output=(256, 256), interpolation=1, radius="max")
    assert dev_writes == [] and [p.rsplit("/", 1)[1] for p in host_writes] == ["m.jpg", "w.jpg", "p.png", "h.jpg"]
    assert _pil((tmp_path / "h.jpg").read_bytes()).size == (512, 256) and _pil((tmp_path / "w.jpg").read_bytes()).size == (512, 256)
