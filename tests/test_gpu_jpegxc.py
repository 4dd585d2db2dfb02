"""The lossless JPEG transcoder on the MI355X through its Python entries -- ``transcode_jpeg``, ``split_sbs_jpeg``, ``swap_sbs_jpeg`` --
against the restatement (jpgxc_ref.py), byte for byte; and the routes that end in a VR180 photo at 512 x 256:
``apply_lr(..., device_jpeg="vr180")``, ``xmp --device`` and ``swap --lossless`` on a side-by-side file written by ``--device-jpeg``."""
import numpy as np
import pytest
import torch
from typer.testing import CliRunner

import jpgdec_ref as D
import jpgxc_cases as K
import jpgxc_ref as X

pytestmark = pytest.mark.gpu
CASES = K.cases()
runner = CliRunner()


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")


def _coefficients(data):
    d = D.decode(data, check=False)
    return d.info, D.dc_values(d.info, d.coef)


@pytest.mark.parametrize("name", ["minus1_last_two_columns_420", "unaligned_size_444", "source_dri7_gray", "source_dri2_422", "noise_q100_gray_crop"])
def test_crop_equals_restatement(name):
    import vr180_convert_amd as V

    data, outputs = CASES[name]
    src = X.Source(data)
    sx, sy, nx, ny, _, _ = outputs[0]["regions"][0]
    crop = (sx * src.mw, sy * src.mh, outputs[0]["width"], outputs[0]["height"])
    for kw in (dict(), dict(optimize=True), dict(restart_mcus=0), dict(restart_mcus=1, optimize=True)):
        assert V.transcode_jpeg(data, crop=crop, **kw) == X.transcode_jpeg(data, crop=crop, **kw), (name, kw)
    assert V.transcode_jpeg(data) == X.transcode_jpeg(data)


@pytest.mark.parametrize("name", ["swap_2x2_gray", "swap_2x2_420", "swap_2x2_422", "noise_q100_444_swap", "swap_dri7_444", "noise_q100_420_split"])
def test_split_and_swap_equal_restatement(name, tmp_path):
    import vr180_convert_amd as V
    from vr180_convert_amd.jpeg_transcode_device import last_transcode_report

    data = CASES[name][0]
    for kw in (dict(), dict(optimize=True, restart_mcus=3)):
        assert V.swap_sbs_jpeg(data, **kw) == X.swap_sbs_jpeg(data, **kw)
        assert V.split_sbs_jpeg(data, **kw) == X.split_sbs_jpeg(data, **kw)
    rep = last_transcode_report()
    assert len(rep["sizes"]) == 2 and rep["rounds"] >= 1
    # swapping twice gives the file's coefficients back; a path is taken as bytes are
    p = tmp_path / "sbs.jpg"
    p.write_bytes(data)
    twice = V.swap_sbs_jpeg(V.swap_sbs_jpeg(p))
    assert np.array_equal(_coefficients(twice)[1], _coefficients(data)[1])


def _sbs_tensor():
    import vr180_convert_amd as V
    from vr180_convert_amd.synth import noise_disc
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder, PolynomialScaler

    left, right = noise_disc(256, 256, 0), noise_disc(256, 256, 1)
    t = EquirectangularEncoder() * PolynomialScaler([0, 1, -0.1]) * FisheyeDecoder("equidistant")
    kw = dict(size_output=(256, 256), interpolation=1, radius="max")
    dev = torch.device("cuda", 0)
    sbs = V.apply_lr_tensors(t, torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev), **kw)
    return t, left, right, kw, sbs


def test_apply_lr_writes_a_vr180_photo_of_the_two_encoded_halves(tmp_path):
    import vr180_convert_amd as V
    from vr180_convert_amd.calibration_cv import vr180_xmp_properties
    from vr180_convert_amd.vr180_photo import read_vr180_photo

    t, left, right, kw, sbs = _sbs_tensor()
    assert tuple(sbs.shape) == (256, 512, 3)
    for extra, enc in ((dict(), dict()), (dict(device_jpeg_optimize=True), dict(optimize=True))):
        out = tmp_path / "photo.jpg"
        V.apply_lr(t, left_path=left, right_path=right, out_path=out, device_jpeg="vr180", **kw, **extra)
        got_l, got_r, props = read_vr180_photo(out.read_bytes())
        want = V.encode_jpeg_tensors([sbs[:, :256], sbs[:, 256:]], **enc)
        assert [got_l, got_r] == want
        assert props == vr180_xmp_properties(512, 256)
    with pytest.raises(ValueError, match="out_path"):
        V.apply_lr(t, left_path=left, right_path=right, out_path=tmp_path / "photo.png", device_jpeg="vr180", **kw)


def test_cli_xmp_device_and_swap_lossless_on_a_device_written_file(tmp_path):
    from vr180_convert_amd import _io, cli
    from vr180_convert_amd.synth import noise_disc
    from vr180_convert_amd.vr180_photo import read_vr180_photo

    l, r = tmp_path / "L.png", tmp_path / "R.png"
    _io.imwrite(l, noise_disc(256, 256, 0))
    _io.imwrite(r, noise_disc(256, 256, 1))
    sbs = tmp_path / "sbs.jpg"
    res = runner.invoke(cli.app, ["lr", str(l), str(r), "--radius", "max", "--size", "256x256", "--interpolation", "inter_linear",
                                  "--out-path", str(sbs), "--device-jpeg"])
    assert res.exit_code == 0, (res.stdout, res.exception)
    data = sbs.read_bytes()
    s, coef = _coefficients(data)
    assert (s.h, s.w, s.hs, s.vs) == (256, 512, 2, 2)
    mcus = coef.reshape(s.mcuy, s.mcux, s.bpm, 64)
    # xmp --device: the left eye is the file, the embedded right eye holds the source's right-half coefficients
    res = runner.invoke(cli.app, ["xmp", "--device", str(sbs)])
    assert res.exit_code == 0, (res.stdout, res.exception)
    got_l, got_r, props = read_vr180_photo((tmp_path / "sbs.xmp.jpg").read_bytes())
    for eye, half in ((got_l, mcus[:, :16]), (got_r, mcus[:, 16:])):
        t, c = _coefficients(eye)
        assert (t.h, t.w) == (256, 256) and np.array_equal(c.reshape(16, 16, 6, 64), half)
    assert (got_l, got_r) == X.split_sbs_jpeg(data)
    assert dict((n, v) for _, n, v in props)["FullPanoWidthPixels"] == 512
    # swap --lossless: the halves exchanged, no coefficient changed; again: the file's coefficients
    res = runner.invoke(cli.app, ["swap", "--lossless", "--no-overwrite", str(sbs)])
    assert res.exit_code == 0, (res.stdout, res.exception)
    swapped = (tmp_path / "sbs.swap.jpg").read_bytes()
    assert swapped == X.swap_sbs_jpeg(data) and sbs.read_bytes() == data
    assert np.array_equal(_coefficients(swapped)[1].reshape(16, 32, 6, 64), np.concatenate([mcus[:, 16:], mcus[:, :16]], axis=1))
    res = runner.invoke(cli.app, ["swap", "--lossless", str(sbs)])
    assert res.exit_code == 0 and sbs.read_bytes() == swapped
    # lr --device-vr180 writes the photo itself
    photo = tmp_path / "photo.jpg"
    res = runner.invoke(cli.app, ["lr", str(l), str(r), "--radius", "max", "--size", "256x256", "--interpolation", "inter_linear",
                                  "--out-path", str(photo), "--device-vr180"])
    assert res.exit_code == 0, (res.stdout, res.exception)
    pl, pr, _ = read_vr180_photo(photo.read_bytes())
    assert _coefficients(pl)[0].w == 256 and _coefficients(pr)[0].w == 256
