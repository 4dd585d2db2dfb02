"""The colour match of the two eyes on the MI355X: every named case of tests/colormatch_cases.py and a
512 x 512 pair that more than one workgroup flushes, byte for byte against the restatement (tests/colormatch_ref.py) -- histograms,
tables, report and result, and every byte around the eyes --, the exact recovery through ``match_eyes_tensors``, a graph capture
replayed on other contents, and ``match_colors=`` through ``apply_lr_tensors`` and ``apply_lr``'s writers."""
import functools

import numpy as np
import pytest
import torch

import colormatch_cases as CC
import colormatch_ref as R

pytestmark = pytest.mark.gpu
NAMES = sorted(CC.shared_cases())


def _views(case, base_t):
    h, w, cn = case.shape
    return [torch.as_strided(base_t, (h, w, cn), (p, cn, 1), off) for off, p in (case.left, case.right)]


def _run(case):
    """the case through the three tensor entries: (result, luts, report, histograms, the base afterwards)"""
    from vr180_convert_amd import colormatch

    base_t = torch.from_numpy(case.base.copy()).cuda()
    left, right = _views(case, base_t)
    ws = torch.full((2, 3, 256), -1, dtype=torch.int32, device="cuda")  # (not zero: the chain zeroes it)
    luts, report = colormatch.color_match_luts_tensor(left, right, workspace=ws, **case.kw)
    tgt = right if case.target == "right" else left
    if case.inplace:
        out = colormatch.apply_luts_tensor(tgt, luts, out=tgt)
        assert out is tgt
    else:
        out = colormatch.apply_luts_tensor(tgt, luts)
    torch.cuda.synchronize()
    return out.cpu().numpy(), luts.cpu().numpy(), report.cpu().numpy(), ws.cpu().numpy().view(np.uint32), base_t.cpu().numpy()


def same(got, want, case):
    result, luts, report, hist, base = got
    wresult, wluts, wreport, whist = want
    assert np.array_equal(hist, whist)
    assert np.array_equal(luts, wluts)
    assert np.array_equal(report, wreport), (report, wreport)
    assert np.array_equal(result, wresult)
    assert np.array_equal(base, CC.expected_base(case, wresult))


# the two the issue names as the likeliest to fail come first in the file
def test_graph_replay_starts_from_a_zeroed_workspace():
    from vr180_convert_amd import colormatch

    pairs = [CC.recovery_pair(3), CC.recovery_pair(4)]
    left, right = (torch.zeros((67, 131, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    ws = torch.zeros((2, 3, 256), dtype=torch.int32, device="cuda")
    out = torch.zeros_like(right)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        left.copy_(torch.from_numpy(pairs[0][0]).cuda())
        right.copy_(torch.from_numpy(pairs[0][1]).cuda())
        with torch.cuda.graph(g, stream=side):
            luts, report = colormatch.color_match_luts_tensor(left, right, workspace=ws, min_pixels=16)
            colormatch.apply_luts_tensor(right, luts, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for L, Rr in pairs + pairs[:1]:
        left.copy_(torch.from_numpy(L).cuda())
        right.copy_(torch.from_numpy(Rr).cuda())
        g.replay()
        torch.cuda.synchronize()
        wluts, wreport, whist = R.luts(L, Rr, **dict(R.DEFAULTS, min_pixels=16))
        assert np.array_equal(ws.cpu().numpy().view(np.uint32), whist)  # this replay's contents alone
        assert np.array_equal(luts.cpu().numpy(), wluts) and np.array_equal(report.cpu().numpy(), wreport)
        assert np.array_equal(out.cpu().numpy(), L) and np.array_equal(right.cpu().numpy(), Rr)


@pytest.mark.parametrize("name", NAMES)
def test_named_case_equals_restatement(name):
    case = CC.shared_cases()[name]
    same(_run(case), CC.reference(name), case)


@functools.lru_cache(maxsize=None)
def _big():
    """512 x 512 per eye as the halves of a 1025-wide side-by-side frame: 16 896 items, 66 workgroups"""
    L = CC.noise_disc(512, 512, 3, 77, hi=200)
    return CC.carve(L, CC.brighter(L), sbs=True, pad=3, off=1)


@pytest.mark.parametrize("kw", [{}, dict(mode="gain"), dict(reference="right")], ids=["histogram", "gain", "right_reference"])
def test_more_than_one_workgroup_flushes(kw):
    case = _big()._replace(kw=kw)
    same(_run(case), CC.reference_of(case), case)


def test_exact_recovery_through_match_eyes_tensors():
    import vr180_convert_amd as V

    L, Rr = CC.recovery_pair(0)
    left, right = torch.from_numpy(L).cuda(), torch.from_numpy(Rr).cuda()
    got = V.match_eyes_tensors(left, right, min_pixels=16)
    assert got is right
    assert np.array_equal(right.cpu().numpy(), L) and np.array_equal(left.cpu().numpy(), L)
    rep = V.color_match_report(V.color_match_luts_tensor(left, torch.from_numpy(Rr).cuda(), min_pixels=16)[1])
    assert rep.status == 0 and rep.n == int(R.mask(L, Rr).sum()) and rep.channels[0].gain == 0.0
    # out of place, the other reference: the left eye is the target and stays as it is
    left2 = torch.from_numpy(Rr).cuda()
    out = torch.zeros_like(left2)
    assert V.match_eyes_tensors(left2, torch.from_numpy(L).cuda(), out=out, reference="right", min_pixels=16) is out
    assert np.array_equal(out.cpu().numpy(), L) and np.array_equal(left2.cpu().numpy(), Rr)


def test_wide_images_raise_before_any_launch():
    import vr180_convert_amd as V

    for dtype in (torch.uint16, torch.float32):
        t = torch.zeros((8, 8, 3), dtype=dtype, device="cuda")
        with pytest.raises(TypeError, match="uint8"):
            V.color_match_luts_tensor(t, t)
        with pytest.raises(TypeError, match="uint8"):
            V.match_eyes_tensors(t, t)


# ---- through the remap entries ----------------------------------------------------------------------------------------------------------
SPEC = [("equirect_enc", True), ("poly", [0, 1, -0.1]), ("fisheye_dec", "equidistant")]


def _chain():
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder, PolynomialScaler

    return EquirectangularEncoder() * PolynomialScaler([0, 1, -0.1]) * FisheyeDecoder("equidistant")


@functools.lru_cache(maxsize=None)
def _remapped():
    """two noise discs, the right one brighter; the oracle's remap of both and the restatement's match of its halves"""
    from oracle import oracle as O
    from vr180_convert_amd.synth import noise_disc

    left = (noise_disc(256, 256, 0) // 2 + 20).astype(np.uint8) * (noise_disc(256, 256, 0).max(axis=2, keepdims=True) > 0)
    right = CC.brighter(left)
    want = O.apply_lr(SPEC, left, right, size_output=(256, 256), interpolation=O.INTER_LINEAR, radius="max")
    matched = {(m, r): np.concatenate([want[:, :256] if r == "left" else R.match_eyes(want[:, :256], want[:, 256:], mode=m, reference=r)[0],
                                       R.match_eyes(want[:, :256], want[:, 256:], mode=m, reference=r)[0] if r == "left" else want[:, 256:]],
                                      axis=1) for m in ("histogram", "gain") for r in ("left", "right")}
    return left, right, want, matched


@pytest.mark.parametrize("mode, ref", [("histogram", "left"), ("gain", "left"), ("histogram", "right")])
def test_apply_lr_tensors_matches_the_halves_after_the_remap(mode, ref):
    import vr180_convert_amd as V

    left, right, want, matched = _remapped()
    sbs = V.apply_lr_tensors(_chain(), torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), size_output=(256, 256), interpolation=1,
                             radius="max", match_colors=mode, match_reference=ref)
    got = sbs.cpu().numpy()
    keep = slice(0, 256) if ref == "left" else slice(256, 512)
    assert np.array_equal(got[:, keep], want[:, keep])  # the reference half is the oracle's remap
    assert np.array_equal(got, matched[(mode, ref)]) and not np.array_equal(got, want)
    plain = V.apply_lr_tensors(_chain(), torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), size_output=(256, 256), interpolation=1,
                               radius="max")
    assert np.array_equal(plain.cpu().numpy(), want)


def test_apply_lr_writes_the_matched_pixels(tmp_path):
    import vr180_convert_amd as V
    from vr180_convert_amd import _io

    left, right, want, matched = _remapped()
    kw = dict(left_path=left, right_path=right, size_output=(256, 256), interpolation=1, radius="max", match_colors="histogram")
    V.apply_lr(_chain(), out_path=tmp_path / "host.png", **kw)
    assert np.array_equal(np.asarray(_io.imread(tmp_path / "host.png")), matched[("histogram", "left")])
    V.apply_lr(_chain(), out_path=tmp_path / "dev.png", device_png=True, **kw)
    assert np.array_equal(np.asarray(_io.imread(tmp_path / "dev.png")), matched[("histogram", "left")])
    V.apply_lr(_chain(), out_path=tmp_path / "dev.jpg", device_jpeg=True, **kw)
    assert (tmp_path / "dev.jpg").read_bytes() == bytes(V.encode_jpeg_tensor(torch.from_numpy(matched[("histogram", "left")]).cuda()))
