"""The device JPEG decoder on the MI355X through the package: the reference's own 2048 x 2048 sample (one entropy-coded segment of
940 KB: the synchronisation rounds carry the whole decode) against Pillow, the round trip through the device encoder, and
``device_decode=True`` in apply_lr, apply and the command line."""
import io
from pathlib import Path

import numpy as np
import pytest
import torch

import jpgdec_cases as DC
import jpgdec_ref as D
import sphere_scene

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
DOCS_JPG = ROOT / "tests" / "golden" / "ref_docs" / "test.jpg"


def _pillow_bgr(data):
    from PIL import Image

    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])


@pytest.fixture(scope="module")
def V():
    import vr180_convert_amd as V

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    return V


@pytest.fixture(scope="module")
def chain():
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder, PolynomialScaler

    return EquirectangularEncoder() * PolynomialScaler([0, 1, -0.1]) * FisheyeDecoder("equidistant")


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """two 256 x 256 JPEG files of fisheye-like discs, a side-by-side file of both, and a progressive one"""
    from vr180_convert_amd.synth import noise_disc

    d = tmp_path_factory.mktemp("jpegdec")
    # (a black frame around the disc: radius="auto" needs black at both ends of the centre row, also behind the JPEG's ringing)
    left, right = (np.pad(noise_disc(208, 208, f), ((24, 24), (24, 24), (0, 0))) for f in (0, 1))
    (d / "l.jpg").write_bytes(DC.pillow(left, 92, "420"))
    (d / "r.jpeg").write_bytes(DC.pillow(right, 92, "444"))
    (d / "sbs.jpg").write_bytes(DC.pillow(np.concatenate([left, right], axis=1), 92, "422"))
    (d / "p.jpg").write_bytes(DC.pillow(left, 92, "420", progressive=True))
    return d


def test_docs_image_equals_pillow(V):
    """test_jpegdec_host.py records the restatement's distance from Pillow: 0 -- so the device equals Pillow's decode"""
    data = DOCS_JPG.read_bytes()
    got = V.decode_jpeg_tensor(data).cpu().numpy()
    rep = V.last_decode_report()
    assert got.shape == (2048, 2048, 3) and np.array_equal(got, _pillow_bgr(data))
    assert rep["segments"] == 1 and rep["rounds"] >= 2 and rep["path"] == "device" and rep["subsequences"] > 1000
    assert np.array_equal(V.imread_tensor(DOCS_JPG, subseq_bits=4096).cpu().numpy(), got)


def test_round_trip_through_the_device_encoder(V):
    frame = torch.from_numpy(sphere_scene.render(512)).cuda()
    data = V.encode_jpeg_tensor(frame)
    got = V.decode_jpeg_tensor(data).cpu().numpy()
    assert np.array_equal(got, D.decode(data, check=False).pixels)
    assert np.array_equal(got, _pillow_bgr(data))  # (the same PSNR as Pillow's decode of these bytes: the same pixels)
    grey = V.encode_jpeg_tensor(frame[..., 1].contiguous())
    g = V.decode_jpeg_tensor(grey, channels=1)
    assert g.shape == (512, 512) and np.array_equal(g.cpu().numpy(), _pillow_bgr(grey)[..., 0])


def test_errors_are_raised_not_hidden(V):
    with pytest.raises(NotImplementedError):
        V.decode_jpeg_tensor(DC.unsupported_cases()["progressive"])
    with pytest.raises(ValueError):
        V.decode_jpeg_tensor(DC.corrupt_cases()["one_block_too_few"][0])
    with pytest.raises(ValueError):
        V.decode_jpeg_tensor(DC.supported_cases()["size_8x8_420"], channels=1)


def test_apply_lr_with_device_decode(V, chain, pair, tmp_path):
    from vr180_convert_amd import _io

    kw = dict(size_output=(256, 256), interpolation=1, radius=120.0)
    l, r = (V.decode_jpeg_tensor(pair / n).cpu().numpy() for n in ("l.jpg", "r.jpeg"))
    V.apply_lr(chain, left_path=l, right_path=r, out_path=tmp_path / "want.npy", **kw)
    V.apply_lr(chain, left_path=pair / "l.jpg", right_path=pair / "r.jpeg", out_path=tmp_path / "got.npy", device_decode=True, **kw)
    want = np.load(tmp_path / "want.npy")
    assert want.any() and np.array_equal(np.load(tmp_path / "got.npy"), want)
    # with the device encoder behind it: file bytes in, file bytes out
    V.apply_lr(chain, left_path=pair / "l.jpg", right_path=pair / "r.jpeg", out_path=tmp_path / "got.jpg", device_decode=True,
               device_jpeg=True, **kw)
    assert (tmp_path / "got.jpg").read_bytes() == V.encode_jpeg_tensor(torch.from_numpy(want).cuda())
    # one side-by-side file: decoded once, the halves are views
    sbs = V.decode_jpeg_tensor(pair / "sbs.jpg").cpu().numpy()
    V.apply_lr(chain, left_path=sbs[:, :256], right_path=sbs[:, 256:], out_path=tmp_path / "want2.npy", **kw)
    V.apply_lr(chain, left_path=pair / "sbs.jpg", right_path=pair / "sbs.jpg", out_path=tmp_path / "got2.npy", device_decode=True, **kw)
    assert np.array_equal(np.load(tmp_path / "got2.npy"), np.load(tmp_path / "want2.npy"))
    # radius="auto" on the decoded tensors
    V.apply_lr(chain, left_path=l, right_path=r, out_path=tmp_path / "want3.npy", **{**kw, "radius": "auto"})
    V.apply_lr(chain, left_path=pair / "l.jpg", right_path=pair / "r.jpeg", out_path=tmp_path / "got3.npy", device_decode=True,
               **{**kw, "radius": "auto"})
    assert np.array_equal(np.load(tmp_path / "got3.npy"), np.load(tmp_path / "want3.npy"))


def test_apply_with_device_decode_and_a_progressive_file(V, chain, pair, tmp_path, monkeypatch):
    from vr180_convert_amd import _io

    host_reads = []
    real = _io.imread
    monkeypatch.setattr(_io, "imread", lambda p: host_reads.append(Path(p).name) or real(p))
    kw = dict(size_output=(256, 256), interpolation=1, radius=120.0)
    outs = V.apply(chain, in_paths=[pair / "l.jpg", pair / "p.jpg"], out_paths=[tmp_path / "a.npy", tmp_path / "b.npy"], device_decode=True, **kw)
    assert host_reads == ["p.jpg"] and len(outs) == 2
    want = V.apply(chain, in_paths=[V.decode_jpeg_tensor(pair / "l.jpg").cpu().numpy(), real(pair / "p.jpg")], **kw)
    for o, w, n in zip(outs, want, ("a.npy", "b.npy")):
        assert w.any() and np.array_equal(o.cpu().numpy(), w) and np.array_equal(np.load(tmp_path / n), w)


def test_cli_device_decode(V, pair, tmp_path):
    """``v1c s in.jpg --device-decode --size 256x256`` writes the same file as the Python call"""
    from typer.testing import CliRunner

    from vr180_convert_amd import cli

    r = CliRunner().invoke(cli.app, ["s", str(pair / "l.jpg"), "--device-decode", "--size", "256x256", "--out-path", str(tmp_path / "cli.png")])
    assert r.exit_code == 0, r.output
    V.apply(cli.parse_transformer(""), in_paths=[pair / "l.jpg"], out_paths=[tmp_path / "py.png"], size_output=(256, 256),
            radius=cli.parse_radius("auto"), device_decode=True)
    assert (tmp_path / "cli.png").stat().st_size > 1000 and (tmp_path / "cli.png").read_bytes() == (tmp_path / "py.png").read_bytes()
    # without the flag the host reader (Pillow: libjpeg-turbo's default decode) gives the same pixels, hence the same file
    r = CliRunner().invoke(cli.app, ["s", str(pair / "l.jpg"), "--size", "256x256", "--out-path", str(tmp_path / "host.png")])
    assert r.exit_code == 0, r.output
    assert (tmp_path / "host.png").read_bytes() == (tmp_path / "cli.png").read_bytes()
