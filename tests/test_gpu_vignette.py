"""The vignetting correction on the MI355X: every named case of tests/vignette_cases.py, byte for byte
against the restatement (tests/vignette_ref.py) -- the result, the ring record and every byte around the image --, the strip whose
table position needs 64 bits, the saturated frame whose ring sums pass 2^32, ``fit_vignette`` on a flat field and on a frame the mask
empties, ``vignette=`` through the remap entries against the composition it stands for, and a graph capture replayed on new pixels."""
import functools

import numpy as np
import pytest
import torch

import vignette_cases as VC
import vignette_ref as R

pytestmark = pytest.mark.gpu
NAMES = sorted(VC.shared_cases())


def _view(case, base_t):
    h, w, cn = case.shape
    es = np.dtype(case.dtype).itemsize
    typed = base_t if es == 1 else base_t[: base_t.numel() // 2 * 2].view(torch.uint16)
    return torch.as_strided(typed, (h, w, cn), (case.pitch // es, cn, 1), case.off // es)


def _run(case):
    """the case through the tensor entries: (result, ring record, the base afterwards)"""
    from vr180_convert_amd import vignette as V

    base_t = torch.from_numpy(case.base.copy()).cuda()
    img = _view(case, base_t)
    rec = V.vignette_rings_tensor(img, center=case.center, radius=case.radius, rings=case.rings, lo=case.lo, hi=case.hi)
    if case.inplace:
        out = V.apply_vignette_tensor(img, case.vignette(), center=case.center, radius=case.radius, out=img)
        assert out is img
    else:
        out = V.apply_vignette_tensor(img, case.vignette(), center=case.center, radius=case.radius)
    torch.cuda.synchronize()
    return out.cpu().numpy(), rec.cpu().numpy(), base_t.cpu().numpy()


def same(got, want, case):
    result, rec, base = got
    wresult, wrec = want
    assert np.array_equal(rec, wrec)
    assert np.array_equal(result, wresult)
    assert np.array_equal(base, VC.expected_base(case, wresult))


@pytest.mark.parametrize("name", NAMES)
def test_named_case_equals_restatement(name):
    case = VC.shared_cases()[name]
    same(_run(case), VC.reference(name), case)


def test_strip_needs_the_64_bit_position():
    """2 x 32767 with the centre at the far end: r2 passes 2^30 and r2 * scale 2^59"""
    case = VC.carve(VC.noise(2, 32767, 3, np.uint16, 50), center=(32766, 1), radius=33000.0, rings=1024)
    cx, cy, scale, shift, _ = VC.geometry(case)
    assert int(R.r2_of(2, 32767, cx, cy).max()) * scale > 1 << 59
    same(_run(case), VC.reference_of(case), case)


def test_saturated_frame_passes_two_to_the_32():
    """1200 x 1200 uint16 of all 65535 in 16 rings: the populated rings' sums pass 2^32, the overflow case of the 32-bit copies in LDS"""
    case = VC.carve(np.full((1200, 1200, 3), 65535, np.uint16), radius=900.0, rings=16, hi=65535)
    want = VC.reference_of(case)
    assert (want[1][:, :3] > 1 << 32).sum() == 3 * 9
    same(_run(case), want, case)


@functools.lru_cache(maxsize=None)
def _big():
    """700 x 1500 uint8 noise around an off-centre circle of 256 rings: 65 800 items, 258 workgroups that each flush"""
    return VC.carve(VC.noise(700, 1500, 3, np.uint8, 51), radius=800.0, rings=256, center=(700, 300))


def test_more_than_one_workgroup_flushes():
    same(_run(_big()), VC.reference_of(_big()), _big())


def test_tables_are_reused_across_frames():
    from vr180_convert_amd import vignette as V

    case = VC.shared_cases()["cn3_uint16"]
    tab = V.tables_tensor(case.vignette(), "cuda")
    assert tab.shape == (3, 1025) and tab.dtype == torch.uint16
    for seed in (1, 2):
        img = VC.noise(37, 83, 3, np.uint16, seed)
        got = V.apply_vignette_tensor(torch.from_numpy(img).cuda(), None, center=case.center, radius=case.radius, tables=tab)
        cx, cy, scale, shift, _ = VC.geometry(case)
        assert np.array_equal(got.cpu().numpy(), R.apply(img, VC.tables(case), cx, cy, scale, shift))
    with pytest.raises(ValueError, match="tables"):
        V.apply_vignette_tensor(torch.from_numpy(img).cuda(), None, radius=44.0, tables=tab[:, :1024].contiguous())


def test_float32_raises_before_any_launch():
    import vr180_convert_amd as V

    t = torch.zeros((8, 8, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(TypeError, match="uint8 and uint16"):
        V.apply_vignette_tensor(t, V.Vignette(), radius=4.0)
    with pytest.raises(TypeError, match="uint8 and uint16"):
        V.vignette_rings_tensor(t, radius=4.0)


# ---- the fit --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_fit_vignette_on_a_flat_field(dtype):
    """the device's statistics are the restatement's, so the fit is the host test's: the coefficients' sum (V at the rim) comes back"""
    import vr180_convert_amd as V
    from vr180_convert_amd import vignette as VG

    truth = VC.carve(np.zeros((1, 1, 3), dtype), coefs=VC.STRONG).vignette()
    top = 255 if dtype == np.uint8 else 65535
    flat = VC.flat_field(truth, 257, 257, (128, 127), 126.0, 0.8 * top, dtype, 3, sigma=0.004 * top)
    fit = V.fit_vignette(torch.from_numpy(flat).cuda(), center=(128, 127), radius=126.0)
    lo, hi = VG.default_mask(dtype)
    want = VG.fit_rings(R.rings(flat, 128, 127, 126 * 126, 256, lo, hi))
    assert (fit.blue, fit.green, fit.red) == (want.blue, want.green, want.red)
    for got, k in zip((fit.blue, fit.green, fit.red), VC.STRONG[0]):
        assert abs(sum(got) - sum(k)) < 0.02
    # the circle fitted on the device: the same model within the fit's own noise
    auto = V.fit_vignette(flat, center="auto", radius="fit")
    assert abs(sum(auto.green) - sum(VC.STRONG[0][1])) < 0.05


def test_a_masked_out_frame_raises_and_counts_nothing():
    import vr180_convert_amd as V

    img = torch.zeros((37, 83, 3), dtype=torch.uint8, device="cuda")
    rec = V.vignette_rings_tensor(img, radius=44.0, rings=64)
    assert rec.shape == (64, 4) and rec.dtype == torch.int64 and not rec.any().item()
    with pytest.raises(ValueError, match="rings hold"):
        V.fit_vignette(img, radius=44.0)
    with pytest.raises(ValueError, match="rings hold"):
        V.fit_vignette(torch.full((37, 83, 3), 200, dtype=torch.uint8, device="cuda"), radius=44.0, lo=10, hi=100)


# ---- through the remap entries ----------------------------------------------------------------------------------------------------------
def _chain(poly=(0, 1, -0.1)):
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder, PolynomialScaler

    return EquirectangularEncoder() * PolynomialScaler(list(poly)) * FisheyeDecoder("equidistant")


def _host_chain():
    """a chain that is not lowered: its map comes from its own NumPy transform (the 'lut' family)"""
    from vr180_convert_amd.chain import TransformerBase

    class Shear(TransformerBase):
        def transform(self, x, y, **kwargs):
            return x + 0.15 * y, y * 0.95

        def inverse_transform(self, x, y, **kwargs):
            return x - 0.15 * y / 0.95, y / 0.95

    return Shear()


def _model():
    return VC.carve(np.zeros((1, 1, 3), np.uint8), coefs=VC.STRONG).vignette()


@pytest.mark.parametrize("family", ["pair", "single", "uint16", "lut"])
def test_remap_tensors_with_vignette_is_the_composition(family):
    """remap_tensors(..., vignette=v) == remap_tensors of apply_vignette_tensor(src, v), byte for byte, one chain per kernel family, and
    last_launch_kinds() does not see the option; the caller's tensors are unchanged"""
    import vr180_convert_amd as V
    from vr180_convert_amd import remapper

    v = _model()
    dtype = np.uint16 if family == "uint16" else np.uint8
    n = 2 if family == "pair" else 1
    srcs_np = [VC.noise(160, 160, 3, dtype, 60 + k, lo=0) for k in range(n)]
    srcs = [torch.from_numpy(a).cuda() for a in srcs_np]
    chain = _host_chain() if family == "lut" else _chain()
    kw = dict(radius=77.5, interpolation=1, center=(81.25, 78.5))
    shape = (96, 128, 3)
    got = [torch.zeros(shape, dtype=srcs[0].dtype, device="cuda") for _ in range(n)]
    paths = V.remap_tensors(chain, srcs, got, vignette=v, **kw)
    kinds = remapper.last_launch_kinds()
    pre = [V.apply_vignette_tensor(s, v, center=kw["center"], radius=kw["radius"]) for s in srcs]
    want = [torch.zeros(shape, dtype=srcs[0].dtype, device="cuda") for _ in range(n)]
    assert V.remap_tensors(chain, pre, want, **kw) == paths and remapper.last_launch_kinds() == kinds
    assert family != "lut" or paths == ["lut"]
    for g, w_, s, a in zip(got, want, srcs, srcs_np):
        assert np.array_equal(g.cpu().numpy(), w_.cpu().numpy()) and g.cpu().numpy().any()
        assert np.array_equal(s.cpu().numpy(), a)
    plain = [torch.zeros(shape, dtype=srcs[0].dtype, device="cuda") for _ in range(n)]
    V.remap_tensors(chain, srcs, plain, **kw)
    assert not np.array_equal(plain[0].cpu().numpy(), got[0].cpu().numpy())
    # one model per unit
    if n == 2:
        v2 = V.Vignette((-0.2, 0.0, 0.0), gamma=2.2)
        V.remap_tensors(chain, srcs, got, vignette=[v, v2], **kw)
        pre[1] = V.apply_vignette_tensor(srcs[1], v2, center=kw["center"], radius=kw["radius"])
        V.remap_tensors(chain, pre, want, **kw)
        assert all(np.array_equal(g.cpu().numpy(), w_.cpu().numpy()) for g, w_ in zip(got, want))


@functools.lru_cache(maxsize=None)
def _eyes():
    """two vignetted discs on black, the right one off centre and darker at the rim"""
    truth_l, truth_r = _model(), VC.carve(np.zeros((1, 1, 3), np.uint8), coefs=VC.ENCODED).vignette()
    left = VC.flat_field(truth_l, 256, 256, (128, 128), 120.0, 200.0, np.uint8, 7, sigma=6.0)
    right = VC.flat_field(truth_r, 256, 256, (124, 131), 118.0, 200.0, np.uint8, 8, sigma=6.0)
    return left, right, truth_l, truth_r


def test_apply_lr_tensors_takes_a_model_per_eye_with_fitted_circles():
    import vr180_convert_amd as V
    from vr180_convert_amd import circle, remapper

    left, right, vl, vr = _eyes()
    lt, rt = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    got = V.apply_lr_tensors(_chain(), lt, rt, size_output=(128, 128), interpolation=1, radius="fit", center="auto", vignette=(vl, vr))
    fits = remapper.fit_circles([lt, rt])
    centers = [circle.round_center(f.cx, f.cy) for f in fits]
    radius = max(circle.round_radius(f.radius) for f in fits)
    pre = [V.apply_vignette_tensor(t, v, center=c, radius=radius) for t, v, c in zip((lt, rt), (vl, vr), centers)]
    want = V.apply_lr_tensors(_chain(), pre[0], pre[1], size_output=(128, 128), interpolation=1, radius=radius, center=centers)
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    assert np.array_equal(lt.cpu().numpy(), left) and np.array_equal(rt.cpu().numpy(), right)  # the caller's eyes are as they were
    # the exact form of radius="auto": resolved once, on the eyes as they came
    got = V.apply_lr_tensors(_chain(), lt, rt, size_output=(128, 128), interpolation=1, radius="auto", vignette=vl)
    r = remapper.get_radius_smart("auto", [lt, rt])
    pre = [V.apply_vignette_tensor(t, vl, radius=r) for t in (lt, rt)]
    want = V.apply_lr_tensors(_chain(), pre[0], pre[1], size_output=(128, 128), interpolation=1, radius=r)
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    with pytest.raises(NotImplementedError, match="auto_radius_on_device"):
        V.apply_lr_tensors(_chain(), lt, rt, size_output=(128, 128), radius="auto", auto_radius_on_device=True, vignette=vl)


def test_vignette_goes_with_chromatic_and_match_colors():
    import vr180_convert_amd as V

    left, right, vl, vr = _eyes()
    lt, rt = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    ca = V.ChromaticAberration(red=[0, 1.004], blue=[0, 0.997])
    kw = dict(size_output=(128, 128), interpolation=1, radius=120.0, chromatic=ca, match_colors="gain")
    got = V.apply_lr_tensors(_chain(), lt, rt, vignette=(vl, vr), **kw)
    pre = [V.apply_vignette_tensor(t, v, radius=120.0) for t, v in zip((lt, rt), (vl, vr))]
    want = V.apply_lr_tensors(_chain(), pre[0], pre[1], **kw)
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    assert np.array_equal(lt.cpu().numpy(), left) and np.array_equal(rt.cpu().numpy(), right)


def test_apply_and_apply_lr_on_host_arrays(tmp_path):
    import vr180_convert_amd as V
    from vr180_convert_amd import _io

    left, right, vl, vr = _eyes()
    keep = left.copy(), right.copy()
    res = V.apply(_chain(), in_paths=[left, right], size_output=(128, 128), interpolation=1, radius=120.0, vignette=vl)
    pre = [V.apply_vignette_tensor(torch.from_numpy(a).cuda(), vl, radius=120.0) for a in (left, right)]
    want = V.apply(_chain(), in_paths=pre, size_output=(128, 128), interpolation=1, radius=120.0)
    for g, w_ in zip(res, want):
        assert np.array_equal(np.asarray(g), w_.cpu().numpy())
    V.apply_lr(_chain(), left_path=left, right_path=right, out_path=tmp_path / "o.png", size_output=(128, 128), interpolation=1,
               radius=120.0, vignette=(vl, vr))
    pre = [V.apply_vignette_tensor(torch.from_numpy(a).cuda(), v, radius=120.0) for a, v in zip((left, right), (vl, vr))]
    want = V.apply_lr_tensors(_chain(), pre[0], pre[1], size_output=(128, 128), interpolation=1, radius=120.0)
    assert np.array_equal(np.asarray(_io.imread(tmp_path / "o.png")), want.cpu().numpy())
    assert np.array_equal(left, keep[0]) and np.array_equal(right, keep[1])
    # tensors of the caller's are never written, either
    lt = torch.from_numpy(left).cuda()
    V.apply(_chain(), in_paths=[lt], size_output=(128, 128), interpolation=1, radius=120.0, vignette=vl)
    assert np.array_equal(lt.cpu().numpy(), left)
    with pytest.raises(TypeError, match="one Vignette"):
        V.apply(_chain(), in_paths=[left, right], size_output=(128, 128), radius=120.0, vignette=[vl, vr])


def test_graph_capture_of_vignette_and_remap_replays_on_new_pixels():
    import vr180_convert_amd as V
    from vr180_convert_amd import vignette as VG

    v = _model()
    frames = [VC.noise(160, 160, 3, np.uint8, 70 + k, lo=0) for k in range(3)]
    src = torch.zeros((160, 160, 3), dtype=torch.uint8, device="cuda")
    dst = torch.zeros((96, 128, 3), dtype=torch.uint8, device="cuda")
    rec = None
    kw = dict(radius=77.5, interpolation=1, center=(81, 78))
    src.copy_(torch.from_numpy(frames[0]).cuda())
    V.remap_tensors(_chain(), [src], [dst], vignette=v, **kw)  # (warm: the plan is made and the model's tables are on the device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            rec = VG.vignette_rings_tensor(src, center=kw["center"], radius=kw["radius"], rings=32, lo=0, hi=255)
            V.remap_tensors(_chain(), [src], [dst], vignette=v, **kw)
    torch.cuda.current_stream().wait_stream(side)
    for a in frames[1:] + frames[:1]:
        src.copy_(torch.from_numpy(a).cuda())
        g.replay()
        torch.cuda.synchronize()
        pre = V.apply_vignette_tensor(torch.from_numpy(a).cuda(), v, center=kw["center"], radius=kw["radius"])
        want = torch.zeros_like(dst)
        V.remap_tensors(_chain(), [pre], [want], **kw)
        assert np.array_equal(dst.cpu().numpy(), want.cpu().numpy())
        assert np.array_equal(rec.cpu().numpy(), R.rings(a, 81, 78, VG.ring_r2(77.5), 32, 0, 255))  # this replay's pixels alone
        assert np.array_equal(src.cpu().numpy(), a)
