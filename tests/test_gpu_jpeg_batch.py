"""The batched device JPEG encoder on the MI355X (``encode_jpeg_tensors`` / ``v1c_jpeg_encode_batch``): images of different size,
channels, quality, subsampling and restart interval in one batch, every file byte for byte the single call's and the restatement's
(jpg_ref.py); pitched views and the halves of one tensor; chunks under a small workspace budget; repeats; two streams; images of
several workgroups in every work list; ``apply`` / ``apply_lr`` / the CLI with ``device_jpeg="batch"``; graph capture.
tests/test_jpeg_batch_host.py runs a sequential copy of the same decomposition on the host, which tells a wrong rule from wrong kernel
plumbing."""
import io

import numpy as np
import pytest
import torch

import jpg_cases as PC
import jpg_ref as R

pytestmark = pytest.mark.gpu
CASES = PC.shared_cases()
NAMES = list(CASES)


@pytest.fixture(scope="module")
def V():
    import vr180_convert_amd as V
    from vr180_convert_amd import _native

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    _native.lib()
    return V


def _view(name):
    """the case as a view of its buffer on the device: pitched rows, the windowed cases behind their odd leads"""
    c = CASES[name]
    base = torch.from_numpy(c.base).cuda()
    return torch.as_strided(base, (c.h, c.w, c.cn), (c.pitch, c.cn, 1), c.offset)


def _params(names):
    return {"quality": [CASES[n].quality for n in names], "subsampling": [CASES[n].subsampling for n in names],
            "restart_mcus": [CASES[n].restart for n in names]}


def _single(V, t, c):
    return V.encode_jpeg_tensor(t, quality=c.quality, subsampling=c.subsampling, restart_mcus=c.restart)


def _first_difference(a, b):
    return len(a), len(b), next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)


@pytest.mark.parametrize("order", ["in_order", "reversed"])
def test_every_file_of_the_batch_is_the_single_calls_and_the_restatements(V, order):
    names = NAMES if order == "in_order" else NAMES[::-1]
    assert len(names) == 48
    views = [_view(n) for n in names]
    assert sum(v.data_ptr() % 2 for v in views) >= 3 and sum(v.stride(0) > v.shape[1] * v.shape[2] for v in views) >= 5  # odd leads, pitched rows
    files = V.encode_jpeg_tensors(views, **_params(names))
    report = V.last_encode_batch_report()
    assert report["chunks"] == 1
    for n, v, f, size in zip(names, views, files, report["sizes"]):
        want = PC.reference(n)[2]
        assert f == want, (n, _first_difference(f, want))
        assert f == _single(V, v, CASES[n]), n
        c = CASES[n]
        assert size == len(want) - len(R.headers(R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart), c.quality)) - 2


def test_halves_of_one_side_by_side_tensor(V):
    """the two eyes of one allocation as two images of a batch: pitched rows, the right one behind a row's half"""
    sbs = torch.from_numpy(PC.smooth(48, 128, 3, 90)).cuda()
    halves = [sbs[:, :64], sbs[:, 64:]]
    assert all(not h.is_contiguous() for h in halves)
    files = V.encode_jpeg_tensors(halves, quality=[95, 80], subsampling=["420", "444"])
    host = sbs.cpu().numpy()
    assert files[0] == R.encode(np.ascontiguousarray(host[:, :64]), 95, "420") and files[1] == R.encode(np.ascontiguousarray(host[:, 64:]), 80, "444")
    assert files[1] == V.encode_jpeg_tensor(halves[1], quality=80, subsampling="444")


def test_small_budget_gives_several_chunks_and_the_same_bytes(V):
    views = [_view(n) for n in NAMES]
    # about 920 bytes of workspace per 8 x 8 block with the counters: 96 x 112 in 4:2:0 has 252 blocks, the 48 cases 2 941
    files = V.encode_jpeg_tensors(views, workspace_budget=600_000, **_params(NAMES))
    chunks = V.last_encode_batch_report()["chunks"]
    assert 4 <= chunks <= 12, chunks
    assert files == [PC.reference(n)[2] for n in NAMES]
    files = V.encode_jpeg_tensors(views, workspace_budget=1, **_params(NAMES))  # smaller than any image: each a chunk of its own
    assert V.last_encode_batch_report()["chunks"] == 48
    assert files == [PC.reference(n)[2] for n in NAMES]


def test_batch_of_one_repeats_and_two_calls(V, tmp_path):
    name = "noise_gray_q100_r1"  # 64 one-block intervals, pads on byte boundaries, a padded last byte of 0xFF: image ends at every kind of pad
    c, want = CASES[name], PC.reference(name)[2]
    t = _view(name)
    kw = {"quality": c.quality, "subsampling": c.subsampling, "restart_mcus": c.restart}
    assert V.encode_jpeg_tensors([t], **kw) == [want]
    assert V.encode_jpeg_tensors([t, t, t], **kw) == [want] * 3
    assert V.encode_jpeg_tensors([t, t, t], **kw) == [want] * 3  # two calls: identical bytes
    assert V.encode_jpeg_tensors([]) == [] and V.last_encode_batch_report() == {"chunks": 0, "sizes": []}
    paths = [tmp_path / f"{k}.jpg" for k in range(2)]
    V.imwrite_jpeg_tensors(paths, [t, _view("bgra")], quality=[c.quality, 95], subsampling="420", restart_mcus=[c.restart, 2])
    assert [p.read_bytes() for p in paths] == [want, PC.reference("bgra")[2]]
    with pytest.raises(ValueError):
        V.encode_jpeg_tensors([t, t], quality=[95])


def test_two_streams_back_to_back(V):
    """two different batches on two streams, no device-wide synchronize in between"""
    a, b = ["noise_q100_420", "size_1x1_gray", "restart1_444"], ["restart2_420", "bgra_odd_lead"]
    va, vb = [_view(n) for n in a], [_view(n) for n in b]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    out = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            out.append(V.encode_jpeg_tensors(va, **_params(a)))
        with torch.cuda.stream(s2):
            out.append(V.encode_jpeg_tensors(vb, **_params(b)))
    torch.cuda.synchronize()
    assert out[0::2] == [[PC.reference(n)[2] for n in a]] * 3
    assert out[1::2] == [[PC.reference(n)[2] for n in b]] * 3


def test_images_of_several_workgroups_in_every_list(V):
    """512 x 512: 4 096 (grey), 12 288 (4:4:4) or 6 144 (4:2:0) blocks -- several workgroups in the 32-block, the 256-block and the
    256-piece list, the last one partial in the piece list and, for the 500 x 508 image, in all three"""
    imgs = [PC.smooth(512, 512, 3, 1), PC.noise(512, 512, 1, 2), PC.noise(500, 508, 3, 3) // 2 + PC.smooth(500, 508, 3, 4) // 2, PC.smooth(512, 512, 1, 5)]
    quality, subsampling = [95, 90, 85, 50], ["420", "420", "444", "444"]
    ts = [torch.from_numpy(a).cuda() for a in imgs]
    files = V.encode_jpeg_tensors(ts, quality=quality, subsampling=subsampling)
    assert V.last_encode_batch_report()["chunks"] == 1
    for t, f, q, s in zip(ts, files, quality, subsampling):
        assert f == V.encode_jpeg_tensor(t, quality=q, subsampling=s)
    assert files[2] == R.encode(imgs[2], 85, "444")


def _chain():
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder, PolynomialScaler

    return EquirectangularEncoder() * PolynomialScaler([0, 1, -0.1]) * FisheyeDecoder("equidistant")


def test_apply_and_the_cli_write_what_the_loop_writes(V, tmp_path):
    from PIL import Image
    from typer.testing import CliRunner

    from vr180_convert_amd import _io, cli
    from vr180_convert_amd.synth import noise_disc

    dev = torch.device("cuda", 0)
    srcs = [noise_disc(96, 96, frame=k) for k in range(3)]
    names = ["a.jpg", "b.png", "c.jpeg"]
    out = {}
    for mode in (True, "batch"):
        d = tmp_path / str(mode)
        d.mkdir()
        res = V.apply(_chain(), in_paths=[torch.from_numpy(s).to(dev) for s in srcs], out_paths=[d / n for n in names], size_output=(64, 48),
                      interpolation=1, radius="max", device_jpeg=mode)
        out[mode] = [(d / n).read_bytes() for n in names]
        assert np.array_equal(np.asarray(Image.open(d / "b.png"))[..., ::-1], res[1].cpu().numpy())
        for k in (0, 2):
            assert out[mode][k] == R.encode(res[k].cpu().numpy(), 95, "420")
    assert out[True] == out["batch"]
    assert V.last_encode_batch_report()["chunks"] == 1 and len(V.last_encode_batch_report()["sizes"]) == 2
    with pytest.raises(ValueError):
        V.apply(_chain(), in_paths=[torch.from_numpy(srcs[0]).to(dev)], out_paths=[tmp_path / "x.jpg"], size_output=(64, 48), device_jpeg="maybe")

    # the CLI: the same files from the flag as from the loop's flag (inputs decoded on the device, so that the results stay there)
    ins = []
    for k, s in enumerate(srcs[:2]):
        ins.append(tmp_path / f"in{k}.jpg")
        _io.imwrite(ins[-1], s)
    got = {}
    for flag in ("--device-jpeg", "--device-jpeg-batch"):
        d = tmp_path / flag.strip("-")
        d.mkdir()
        r = CliRunner().invoke(cli.app, ["s", *[str(p) for p in ins], "--radius", "max", "--size", "64x48", "--interpolation", "inter_linear",
                                         "--out-path", str(d), "--device-decode", flag])
        assert r.exit_code == 0, r.output
        got[flag] = sorted((p.name, p.read_bytes()) for p in d.iterdir())
    assert got["--device-jpeg"] == got["--device-jpeg-batch"] and [n for n, _ in got["--device-jpeg"]] == ["in0.jpg", "in1.jpg"]
    assert all(b"\xff\xdd\x00\x04" in data for _, data in got["--device-jpeg-batch"])  # DRI: the device encoder's file, not the host writer's


def test_apply_lr_batch_equals_the_single_call(V, tmp_path):
    from vr180_convert_amd.synth import noise_disc

    left, right = noise_disc(128, 128, frame=1), noise_disc(128, 128, frame=2)
    files = []
    for mode in (True, "batch"):
        p = tmp_path / f"{mode}.jpg"
        V.apply_lr(_chain(), left_path=left, right_path=right, out_path=p, size_output=(64, 64), interpolation=1, radius="max", device_jpeg=mode)
        files.append(p.read_bytes())
    assert files[0] == files[1] and files[0][:2] == b"\xff\xd8"
    from PIL import Image

    assert Image.open(io.BytesIO(files[1])).size == (128, 64)


def test_graph_capture_is_refused_and_launches_nothing(V):
    t = _view("size_17x17_420")
    want = V.encode_jpeg_tensors([t, t])
    before = V.last_encode_batch_report()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    dummy = torch.zeros(16, device="cuda")
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            dummy.zero_()
            with pytest.raises(NotImplementedError, match="graph"):
                V.encode_jpeg_tensors([t, t])
    torch.cuda.current_stream().wait_stream(s)
    assert V.last_encode_batch_report()["chunks"] == 0 and before["chunks"] == 1  # nothing ran
    assert V.encode_jpeg_tensors([t, t]) == want
