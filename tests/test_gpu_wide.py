"""16-bit and float32 images on the MI355X: every case against the NumPy restatement of cv2's float-weight remap (wide_ref.py) applied
to the oracle's map, with the kernel family it is meant for asserted (``last_launch_kinds``) so that no silent fallback can pass."""
import numpy as np
import pytest
import torch

import chainspecs as CS
import wide_ref as W
from vr180_convert_amd.chain import get_radius

pytestmark = pytest.mark.gpu

RAY = [("equirect_enc", True), ("poly", [0, 1, -0.1]), CS.EQUI]
PLANAR = [("fisheye_enc", "rectilinear"), CS.EQUI]
LITERAL = CS.SMALL_CASES["equirect_decoder"][0]
FIXUP = [CS.SMALL_CASES["back_hemisphere"][0], CS.SMALL_CASES["poly_c0"][0]]
BVS = [70000, -3, 2.5, 1.5, 0.25, (70000, -3, 2.5), (1.5, 0.25, -3, 2.5)]


@pytest.fixture(scope="module")
def V():
    import vr180_convert_amd as V
    from vr180_convert_amd import _native

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    _native.lib()
    return V


@pytest.fixture(scope="module")
def R(V):
    from vr180_convert_amd import remapper

    return remapper


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def disc(dtype, h, w, cn, seed, r=None):
    """A textured disc on black (the border radius="auto" looks for), in the value range of the type: u16 full scale, f32 with
    negatives, values above 1 and a few +-Inf / NaN inside the disc."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    r = r or 0.45 * min(h, w)
    inside = (yy - h / 2) ** 2 + (xx - w / 2) ** 2 < r * r
    if dtype == np.uint16:
        a = rng.integers(0, 65536, (h, w, cn)).astype(np.uint16)
        a[..., 0] = np.maximum(a[..., 0], 1000)
    else:
        a = rng.normal(500.0, 400.0, (h, w, cn)).astype(np.float32)
        a[..., 0] = np.abs(a[..., 0]) + 50
        m = rng.random((h, w))
        a[m < 0.002] = np.inf
        a[(m > 0.002) & (m < 0.004)] = -np.inf
        a[(m > 0.004) & (m < 0.006)] = np.nan
    a[~inside] = 0
    return a


def same(got, want):
    if got.dtype == np.uint16:
        return got.tobytes() == want.tobytes()
    return np.array_equal(got, want, equal_nan=True)


def ndiff(got, want):
    g, w = got.astype(np.float64), want.astype(np.float64)
    return int((~((g == w) | (np.isnan(g) & np.isnan(w)))).sum())


def expected(O, spec, src, *, radius, size_in, out_wh, interp, border, bv, dst=None):
    xm, ym = O.get_map(spec, radius=radius, size_input=size_in, size_output=out_wh)
    return W.remap(src, xm, ym, interp, border, bv, dst=dst)


def run_one(V, dev, spec, src, out_wh, *, interp, border, bv, radius, rotations=None):
    s = torch.from_numpy(src).to(dev)
    d = torch.empty((out_wh[1], out_wh[0], src.shape[2]), dtype=s.dtype, device=dev)
    init = disc(src.dtype.type, out_wh[1], out_wh[0], src.shape[2], 5)
    d.copy_(torch.from_numpy(init))
    run_one.paths = V.remap_tensors(CS.to_product(spec), [s], [d], radius=radius, interpolation=interp, boarder_mode=border,
                                    boarder_value=bv, rotations=rotations)
    torch.cuda.synchronize()
    return d.cpu().numpy(), init


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("interp", [0, 1, 2, 3, 4])
def test_full_matrix_ray_chain(V, R, oracle_mod, dev, dtype, interp):
    case = 0
    for border in range(6):
        for cn in (1, 3, 4):
            src = disc(dtype, 192, 208, cn, 100 + case)
            bv = BVS[case % len(BVS)]
            case += 1
            got, init = run_one(V, dev, RAY, src, (176, 144), interp=interp, border=border, bv=bv, radius=96.0)
            kinds = R.last_launch_kinds()
            want = expected(oracle_mod, RAY, src, radius=96.0, size_in=(192, 208), out_wh=(176, 144), interp=interp, border=border,
                            bv=bv, dst=init)
            assert kinds in (["wide"], ["wide+fixup"]), kinds
            assert same(got, want), (dtype, interp, border, cn, bv, ndiff(got, want))


@pytest.mark.parametrize("name,dtype,spec", [("planar", np.float32, PLANAR), ("literal", np.uint16, LITERAL)])
def test_planar_and_literal_chains(V, R, oracle_mod, dev, name, dtype, spec):
    src = disc(dtype, 160, 160, 3, 7)
    for interp, border in ((1, 0), (4, 4), (2, 5)):
        got, init = run_one(V, dev, spec, src, (150, 130), interp=interp, border=border, bv=(3, 70000, 2.5), radius=80.0)
        kinds = R.last_launch_kinds()
        assert kinds == ["wide"] if name == "literal" else kinds[0].startswith("wide"), kinds
        assert run_one.paths == [name], run_one.paths  # the coordinate producer: MODE_LITERAL, or the fused planar one
        want = expected(oracle_mod, spec, src, radius=80.0, size_in=(160, 160), out_wh=(150, 130), interp=interp, border=border,
                        bv=(3, 70000, 2.5), dst=init)
        assert same(got, want), (name, interp, border, ndiff(got, want))


def test_fixup_pass(V, R, oracle_mod, dev):
    kinds = []
    for k, spec in enumerate(FIXUP):
        src = disc(np.uint16, 256, 256, 3, 11 + k)
        got, init = run_one(V, dev, spec, src, (256, 256), interp=4, border=0, bv=7, radius=128.0)
        kinds += R.last_launch_kinds()
        want = expected(oracle_mod, spec, src, radius=128.0, size_in=(256, 256), out_wh=(256, 256), interp=4, border=0, bv=7, dst=init)
        assert same(got, want), (k, ndiff(got, want))
    assert "wide+fixup" in kinds, kinds


def test_per_unit_rotations(V, R, oracle_mod, dev):
    spec = [("equirect_enc", True), ("rot", CS.ry(0.1)), CS.EQUI]
    rots = [np.array(CS.ry(a)) for a in (0.2, -0.3, 0.05)]
    srcs = [disc(np.float32, 128, 128, 4, 20 + k) for k in range(3)]
    s = [torch.from_numpy(a).to(dev) for a in srcs]
    d = [torch.zeros((112, 120, 4), dtype=torch.float32, device=dev) for _ in srcs]
    V.remap_tensors(CS.to_product(spec), s, d, radius=64.0, interpolation=2, boarder_mode=1, rotations=rots)
    torch.cuda.synchronize()
    assert R.last_launch_kinds()[0].startswith("wide")
    for k in range(3):
        sp = [spec[0], ("rot", rots[k]), spec[2]]
        want = expected(oracle_mod, sp, srcs[k], radius=64.0, size_in=(128, 128), out_wh=(120, 112), interp=2, border=1, bv=0)
        got = d[k].cpu().numpy()
        assert same(got, want), (k, ndiff(got, want))


def test_more_than_16_units(V, R, oracle_mod, dev):
    n = 19
    srcs = [disc(np.uint16, 96, 96, 1, 40 + k) for k in range(n)]
    s = [torch.from_numpy(a).to(dev) for a in srcs]
    d = [torch.zeros((80, 88, 1), dtype=torch.uint16, device=dev) for _ in srcs]
    V.remap_tensors(CS.to_product(RAY), s, d, radius=48.0, interpolation=1, boarder_mode=0, boarder_value=300)
    torch.cuda.synchronize()
    assert R.last_launch_kinds()[0].startswith("wide")
    xm, ym = oracle_mod.get_map(RAY, radius=48.0, size_input=(96, 96), size_output=(88, 80))
    for k in range(n):
        want = W.remap(srcs[k], xm, ym, 1, 0, 300)
        assert same(d[k].cpu().numpy(), want), k


def test_user_transformer_takes_the_lut_path(V, R, dev):
    from vr180_convert_amd.chain import TransformerBase

    class Shear(TransformerBase):
        def transform(self, x, y, **kwargs):
            return x + 0.15 * y, y * 0.95

        def inverse_transform(self, x, y, **kwargs):
            return x - 0.15 * y / 0.95, y / 0.95

    t = Shear()
    for dtype in (np.uint16, np.float32):
        src = disc(dtype, 100, 120, 3, 61)
        s = torch.from_numpy(src).to(dev)
        d = torch.zeros((90, 110, 3), dtype=s.dtype, device=dev)
        V.remap_tensors(t, [s], [d], radius=50.0, interpolation=4, boarder_mode=4)
        torch.cuda.synchronize()
        assert R.last_launch_kinds() == ["lut"]
        xm, ym = R._host_map(t, radius=50.0, size_input=(100, 120), size_output=(110, 90))
        want = W.remap(src, xm, ym, 4, 4, 0)
        got = d.cpu().numpy()
        assert same(got, want), (dtype, ndiff(got, want))


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("ndim", [2, 3])
def test_apply_numpy(V, oracle_mod, dtype, ndim):
    src = disc(dtype, 128, 144, 1 if ndim == 2 else 3, 71)
    img = src[..., 0] if ndim == 2 else src
    out = V.apply(CS.to_product(RAY), in_paths=img, size_output=(120, 100), interpolation=1, radius="max")[0]
    assert out.dtype == dtype and out.shape == ((100, 120) if ndim == 2 else (100, 120, 3))
    want = expected(oracle_mod, RAY, src, radius=64.0, size_in=(128, 144), out_wh=(120, 100), interp=1, border=0, bv=0)
    assert same(out if ndim == 3 else out[..., None], want)


def test_apply_mixed_types_and_cache_keys(V, R, oracle_mod):
    t = CS.to_product(RAY)
    u16 = disc(np.uint16, 128, 128, 3, 81)
    f32 = disc(np.float32, 128, 128, 3, 82)
    u8 = (u16 >> 8).astype(np.uint8)
    outs = V.apply(t, in_paths=[u16, f32, u8], size_output=(100, 90), interpolation=4, radius="max")
    assert [o.dtype for o in outs] == [np.uint16, np.float32, np.uint8]
    xm, ym = oracle_mod.get_map(RAY, radius=64.0, size_input=(128, 128), size_output=(100, 90))
    assert same(outs[0], W.remap(u16, xm, ym, 4, 0, 0))
    assert same(outs[1], W.remap(f32, xm, ym, 4, 0, 0))
    assert np.array_equal(outs[2], oracle_mod.remap(u8, xm, ym, 4, 0, 0))
    # one geometry, first 8-bit then 16-bit (then 8-bit again): the pixel type is part of every plan / memo key
    R.clear_caches()
    for img in (u8, u16, u8, f32):
        out = V.apply(t, in_paths=img, size_output=(100, 90), interpolation=1, radius="max")[0]
        want = oracle_mod.remap(img, xm, ym, 1, 0, 0) if img.dtype == np.uint8 else W.remap(img, xm, ym, 1, 0, 0)
        assert out.dtype == img.dtype
        assert same(out, want) if img.dtype != np.uint8 else np.array_equal(out, want)


def test_apply_lr_arrays_and_odd_sbs(V, oracle_mod, tmp_path):
    t = CS.to_product(RAY)
    left, right = disc(np.uint16, 128, 128, 3, 91), disc(np.uint16, 128, 128, 3, 92)
    V.apply_lr(t, left_path=left, right_path=right, out_path=tmp_path / "a.npy", size_output=(96, 80), interpolation=1, radius="auto")
    got = np.load(tmp_path / "a.npy")
    r = max(get_radius(left), get_radius(right))  # (the reference's NumPy estimate: raw values, any type)
    xm, ym = oracle_mod.get_map(RAY, radius=r, size_input=(128, 128), size_output=(96, 80))
    assert got.dtype == np.uint16 and same(got, np.concatenate([W.remap(left, xm, ym, 1, 0, 0), W.remap(right, xm, ym, 1, 0, 0)], axis=1))
    # one odd-width side-by-side array split in halves (W // 2 and W - W // 2 columns): one map, of the left half's geometry
    sbs = disc(np.uint16, 120, 241, 3, 93)
    lh, rh = sbs[:, :120], sbs[:, 120:]
    V.apply_lr(t, left_path=lh, right_path=rh, out_path=tmp_path / "b.npy", size_output=(96, 80), interpolation=4, radius="max")
    got = np.load(tmp_path / "b.npy")
    xm, ym = oracle_mod.get_map(RAY, radius=60.0, size_input=(120, 120), size_output=(96, 80))
    want = np.concatenate([W.remap(np.ascontiguousarray(lh), xm, ym, 4, 0, 0), W.remap(np.ascontiguousarray(rh), xm, ym, 4, 0, 0)], axis=1)
    assert same(got, want), ndiff(got, want)


def test_apply_lr_merge_and_png(V, oracle_mod, tmp_path):
    from test_wide_host import decode_png

    t = CS.to_product(RAY)
    left, right = disc(np.uint16, 128, 128, 3, 95), disc(np.uint16, 128, 128, 3, 96)
    xm, ym = oracle_mod.get_map(RAY, radius=64.0, size_input=(128, 128), size_output=(96, 80))
    el, er = W.remap(left, xm, ym, 1, 0, 0), W.remap(right, xm, ym, 1, 0, 0)
    V.apply_lr(t, left_path=left, right_path=right, out_path=tmp_path / "m.npy", size_output=(96, 80), interpolation=1, radius="max",
               merge=True)
    got = np.load(tmp_path / "m.npy")
    colors = [(0, 128, 255), (255, 128, 0)]  # the reference's expression, remapper.py:485-497
    want = np.mean(el, axis=-1)[..., None] * np.array(colors[0]).reshape(1, 1, 3) + np.mean(er, axis=-1)[..., None] * np.array(
        colors[1]).reshape(1, 1, 3)
    want /= 255
    # (the float64 anaglyph is written as cv.imwrite writes it: saturated to uint8)
    assert got.dtype == np.uint8 and np.array_equal(got, np.clip(np.rint(want), 0, 255).astype(np.uint8))
    V.apply_lr(t, left_path=left, right_path=right, out_path=tmp_path / "p.png", size_output=(96, 80), interpolation=1, radius="max")
    depth, px = decode_png((tmp_path / "p.png").read_bytes())
    assert depth == 16 and np.array_equal(px, np.concatenate([el, er], axis=1)[..., ::-1])


@pytest.mark.parametrize("radius", ["auto", "max", 57.5])
def test_apply_lr_tensors(V, R, oracle_mod, dev, radius):
    t = CS.to_product(RAY)
    left, right = disc(np.float32, 128, 160, 3, 101, r=50), disc(np.float32, 128, 160, 3, 102, r=54)
    lt, rt = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    out = V.apply_lr_tensors(t, lt, rt, size_output=(96, 80), interpolation=4, radius=radius, auto_radius_on_device=True)
    torch.cuda.synchronize()
    if radius == "auto":
        assert R.last_auto_radius_form() == "exact"
        r = max(get_radius(left), get_radius(right))
    else:
        r = 64.0 if radius == "max" else radius
    assert R.last_launch_kinds()[0].startswith("wide")
    xm, ym = oracle_mod.get_map(RAY, radius=r, size_input=(128, 160), size_output=(96, 80))
    want = np.concatenate([W.remap(left, xm, ym, 4, 0, 0), W.remap(right, xm, ym, 4, 0, 0)], axis=1)
    got = out.cpu().numpy()
    assert out.dtype == torch.float32 and same(got, want), ndiff(got, want)


def test_get_radius_of_a_uint16_tensor(V, R, dev):
    for h, w in ((128, 160), (170, 130)):
        img = disc(np.uint16, h, w, 3, 111, r=0.4 * min(h, w))
        img[img < 20] = 5  # dark but under the threshold on raw values
        assert R.get_radius_smart("auto", [torch.from_numpy(img).to(dev)]) == get_radius(img)


def test_graph_capture_replays_the_eager_result(V, R, oracle_mod, dev):
    from vr180_convert_amd.chain import lower_for_get_map

    src = torch.from_numpy(disc(np.uint16, 128, 128, 3, 121)).to(dev)
    chain = lower_for_get_map(CS.to_product(FIXUP[0]), radius=64.0, size_input=(128, 128), size_output=(112, 96))
    plan = R.Plan(chain, src_hw=(128, 128), dst_wh=(112, 96), cn=3, interpolation=2, border_mode=0, border_value=9, device=dev,
                  dtype=torch.uint16)
    eager = torch.zeros((96, 112, 3), dtype=torch.uint16, device=dev)
    plan.run([src], [eager])
    torch.cuda.synchronize()
    assert plan.last_launch() in ("wide", "wide+fixup")
    out = torch.zeros_like(eager)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            plan.run([src], [out])
    torch.cuda.current_stream(dev).wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_one_type_then_mixed_types_same_geometry(V, R, oracle_mod, dev):
    """A call with one pixel type, then one with several of the same geometry: the second must not take the first one's plan."""
    t = CS.to_product(RAY)
    u16, f32 = disc(np.uint16, 128, 128, 3, 131), disc(np.float32, 128, 128, 3, 132)
    xm, ym = oracle_mod.get_map(RAY, radius=64.0, size_input=(128, 128), size_output=(100, 90))
    su, sf = torch.from_numpy(u16).to(dev), torch.from_numpy(f32).to(dev)
    du, df = torch.zeros((90, 100, 3), dtype=torch.uint16, device=dev), torch.zeros((90, 100, 3), dtype=torch.float32, device=dev)
    for _ in range(2):
        V.remap_tensors(t, [su], [du], radius=64.0, interpolation=1)
    V.remap_tensors(t, [su, sf], [du, df], radius=64.0, interpolation=1)
    torch.cuda.synchronize()
    assert R.last_launch_kinds() == ["wide", "wide"]
    assert same(du.cpu().numpy(), W.remap(u16, xm, ym, 1, 0, 0)) and same(df.cpu().numpy(), W.remap(f32, xm, ym, 1, 0, 0))
    # the same through apply(): one uint16 image, then uint16 + float32 images of that size
    V.apply(t, in_paths=u16, size_output=(100, 90), interpolation=1, radius="max")
    outs = V.apply(t, in_paths=[u16, f32], size_output=(100, 90), interpolation=1, radius="max")
    assert same(outs[0], W.remap(u16, xm, ym, 1, 0, 0)) and same(outs[1], W.remap(f32, xm, ym, 1, 0, 0))
