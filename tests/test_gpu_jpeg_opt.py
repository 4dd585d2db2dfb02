"""The optimised Huffman tables of the device JPEG encoder on the MI355X (``optimize=True``: ``v1c_jpeg_encode_opt`` /
``v1c_jpeg_encode_batch_opt``, csrc/kernels_jpeg_opt.hip): every case of tests/jpg_opt_cases.py against the restatement
(jpg_opt_ref.py) byte for byte and smaller than its standard-table file; a batch that mixes optimising and plain images, grey and
colour, both subsamplings and several restart intervals against the single calls; the device decoder on the optimised files; ``apply``
and the CLI.  tests/test_jpeg_opt_host.py runs the same images through the host build of the symbol walk and the table builder, which
tells a wrong rule from wrong kernel plumbing."""
import io

import numpy as np
import pytest
import torch

import jpg_opt_cases as K
import jpg_ref as R

pytestmark = pytest.mark.gpu
CASES = K.shared_cases()


@pytest.fixture(scope="module")
def V():
    import vr180_convert_amd as V
    from vr180_convert_amd import _native

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    _native.lib()
    return V


def _view(name):
    """the case as a view of its buffer on the device: pitched rows for the half of a side-by-side image"""
    c = CASES[name]
    base = torch.from_numpy(c.base).cuda()
    return torch.as_strided(base, (c.h, c.w, c.cn), (c.pitch, c.cn, 1), c.offset)


def _kw(c, **more):
    return {"quality": c.quality, "subsampling": c.subsampling, "restart_mcus": c.restart, **more}


def _first_difference(a, b):
    return len(a), len(b), next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)


@pytest.mark.parametrize("name", list(CASES))
def test_optimised_file_equals_restatement_and_is_smaller(V, name):
    c = CASES[name]
    t = _view(name)
    _, _, want, std, _ = K.reference(name)
    got = V.encode_jpeg_tensor(t, **_kw(c, optimize=True))
    assert got == want, (name, _first_difference(got, want))
    plain = V.encode_jpeg_tensor(t, **_kw(c))
    assert plain == std and V.encode_jpeg_tensor(t, **_kw(c, optimize=False)) == std
    print(name, "file", len(plain), "->", len(got), "scan", len(K.scan_of(plain)), "->", len(K.scan_of(got)))
    if name == K.FLAT:
        assert len(K.scan_of(got)) == len(K.scan_of(plain)) == 1 and len(got) < len(plain)
    else:
        assert len(got) < len(plain) and len(K.scan_of(got)) < len(K.scan_of(plain))
    assert V.encode_jpeg_tensor(t, **_kw(c, optimize=True)) == got  # two calls: identical bytes


def test_mixed_batch_equals_the_single_calls(V, tmp_path):
    """optimising and plain images, grey and colour, 4:2:0 and 4:4:4, restart intervals of 1, 2, a row and more, a 4-channel image and
    a pitched view in one list"""
    names = ["gray_136_q95_r1", "corner_444_q100", "noise_16x16_420", K.FLAT, "restart1_17x9", "bgra", "right_half", "gray_136_q100",
             "corner_420_q100", "gray_136_q95_r1", "docs_444_q95"]
    optimize = [True, False, True, True, True, False, True, False, True, False, True]
    views = [_view(n) for n in names]
    assert {CASES[n].cn for n in names} == {1, 3, 4} and {CASES[n].subsampling for n in names if CASES[n].cn > 1} == {"420", "444"}
    assert len({CASES[n].restart for n in names}) >= 4 and not views[6].is_contiguous()
    kw = {"quality": [CASES[n].quality for n in names], "subsampling": [CASES[n].subsampling for n in names],
          "restart_mcus": [CASES[n].restart for n in names]}
    files = V.encode_jpeg_tensors(views, optimize=optimize, **kw)
    report = V.last_encode_batch_report()
    assert report["chunks"] == 1  # one chunk: two synchronisations for the whole list, with the tables built on the device in between
    for n, v, f, o, size in zip(names, views, files, optimize, report["sizes"]):
        assert f == V.encode_jpeg_tensor(v, **_kw(CASES[n], optimize=o)), (n, o)
        assert f == K.reference(n)[2 if o else 3], (n, o)
        assert size == len(K.scan_of(f))
    # all optimising, all plain, and one value for all
    assert V.encode_jpeg_tensors(views[:5], optimize=True, **{k: v[:5] for k, v in kw.items()}) == [K.reference(n)[2] for n in names[:5]]
    assert V.encode_jpeg_tensors(views[:5], **{k: v[:5] for k, v in kw.items()}) == [K.reference(n)[3] for n in names[:5]]
    # chunks under a small budget: the same bytes
    small = V.encode_jpeg_tensors(views[:10], optimize=optimize[:10], workspace_budget=300_000, **{k: v[:10] for k, v in kw.items()})
    assert V.last_encode_batch_report()["chunks"] > 1 and small == files[:10]
    paths = [tmp_path / f"{k}.jpg" for k in range(3)]
    V.imwrite_jpeg_tensors(paths, views[:3], optimize=optimize[:3], **{k: v[:3] for k, v in kw.items()})
    assert [p.read_bytes() for p in paths] == files[:3]
    V.imwrite_jpeg_tensor(paths[0], views[0], **_kw(CASES[names[0]], optimize=True))
    assert paths[0].read_bytes() == files[0]
    with pytest.raises(ValueError):
        V.encode_jpeg_tensors(views[:2], optimize=[True])


def test_device_decoder_reads_the_optimised_tables(V):
    for name in ("docs_420_q95", "corner_444_q100", "gray_136_q95_r1", "restart1_17x9"):
        c = CASES[name]
        t = _view(name)
        a = V.decode_jpeg_tensor(V.encode_jpeg_tensor(t, **_kw(c, optimize=True)))
        b = V.decode_jpeg_tensor(V.encode_jpeg_tensor(t, **_kw(c)))
        assert a.shape[:2] == (c.h, c.w) and torch.equal(a, b), name


def test_apply_and_the_cli_write_optimised_files(V, tmp_path):
    from PIL import Image
    from typer.testing import CliRunner

    from vr180_convert_amd import _io, cli
    from vr180_convert_amd.synth import noise_disc
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder, PolynomialScaler

    chain = EquirectangularEncoder() * PolynomialScaler([0, 1, -0.1]) * FisheyeDecoder("equidistant")
    dev = torch.device("cuda", 0)
    srcs = [noise_disc(96, 96, frame=k) for k in range(2)]
    out = {}
    for mode in (True, "batch"):
        d = tmp_path / str(mode)
        d.mkdir()
        res = V.apply(chain, in_paths=[torch.from_numpy(s).to(dev) for s in srcs], out_paths=[d / "a.jpg", d / "b.jpg"], size_output=(64, 48),
                      interpolation=1, radius="max", device_jpeg=mode, device_jpeg_optimize=True)
        out[mode] = [(d / n).read_bytes() for n in ("a.jpg", "b.jpg")]
        for data, r in zip(out[mode], res):
            assert Image.open(io.BytesIO(data)).size == (64, 48)
            assert data == V.encode_jpeg_tensor(r, optimize=True) and len(data) < len(V.encode_jpeg_tensor(r))
    assert out[True] == out["batch"]
    p = tmp_path / "lr.jpg"
    V.apply_lr(chain, left_path=srcs[0], right_path=srcs[1], out_path=p, size_output=(64, 64), interpolation=1, radius="max", device_jpeg=True,
               device_jpeg_optimize=True)
    q = tmp_path / "lr_plain.jpg"
    V.apply_lr(chain, left_path=srcs[0], right_path=srcs[1], out_path=q, size_output=(64, 64), interpolation=1, radius="max", device_jpeg=True)
    assert Image.open(p).size == (128, 64) and p.stat().st_size < q.stat().st_size
    assert np.array_equal(np.asarray(Image.open(p)), np.asarray(Image.open(q)))

    src = tmp_path / "in0.jpg"
    _io.imwrite(src, srcs[0])
    got = {}
    for flags in (["--device-jpeg"], ["--device-jpeg", "--device-jpeg-optimize"], ["--device-jpeg-batch", "--device-jpeg-optimize"]):
        d = tmp_path / "_".join(f.strip("-") for f in flags)
        d.mkdir()
        r = CliRunner().invoke(cli.app, ["s", str(src), "--radius", "max", "--size", "64x48", "--interpolation", "inter_linear", "--out-path", str(d),
                                         "--device-decode", *flags])
        assert r.exit_code == 0, r.output
        got[len(got)] = (d / "in0.jpg").read_bytes()
    assert Image.open(io.BytesIO(got[1])).size == (64, 48) and got[1] == got[2] and len(got[1]) < len(got[0])
    assert b"\xff\xdd\x00\x04" in got[1]  # DRI: the device encoder's file
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(got[1]))), np.asarray(Image.open(io.BytesIO(got[0]))))
