"""radius="auto" -- the reference's default, remapper.py:333,416 -- on every launch path, bit-exact against the C oracle.

The device form (``remap_tensors_auto``: ``v1c_plan_run_auto_images`` / ``v1c_plan_run_auto``) runs kernels without plan-time boxes: they
bound their source boxes themselves for any radius up to 4 x the larger source dimension, and a one-thread kernel writes the Denormalize
scale.  The exact form takes the estimate to the host.  Every case asserts which form and which kernel family served it
(``last_auto_radius_form`` / ``last_launch_kinds``), so that a silent fallback cannot make it pass.
"""
import numpy as np
import pytest
import torch

import chainspecs as CS

pytestmark = pytest.mark.gpu

SPEC_A = [("equirect_enc", True), ("rot", CS.ry(0.2)), ("poly", [0, 1, -0.08]), CS.EQUI]
SPEC_B = [("equirect_enc", True), ("poly", [0, 1, -0.05]), CS.EQUI]
BV = (17, 200, 90, 240)
DEVICE_KINDS = ("tile", "rot_pair", "cn_rot")  # what v1c_plan_run_auto launches (never 'generic', never a fix-up pass)


@pytest.fixture(scope="module")
def V():
    import vr180_convert_amd as V
    from vr180_convert_amd import _native

    _native.lib()
    assert torch.cuda.is_available()
    return V


@pytest.fixture(scope="module")
def R(V):
    from vr180_convert_amd import remapper

    return remapper


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _disc(h, w, r, seed, cn=3, cx=None, cy=None):
    """Noise inside a circle, black outside: get_radius gives about -r (the reference's 180-degree flip quirk)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cx, cy = (w / 2 if cx is None else cx), (h / 2 if cy is None else cy)
    img = rng.integers(40, 256, (h, w, cn), dtype=np.uint8)
    img[(xx - cx) ** 2 + (yy - cy) ** 2 > r * r] = 0
    return img


def _banded(h, w, seed, bands, cn=3):
    """Noise with black bands across get_radius's line (the centre row of a landscape source: column bands; else row bands):
    first band [x0, ...), last band [..., x1) give radius (x1 - x0) / 2 > 0."""
    img = np.random.default_rng(seed).integers(40, 256, (h, w, cn), dtype=np.uint8)
    for a, b in bands:
        if w > h:
            img[:, a:b] = 0
        else:
            img[a:b] = 0
    return img


def _pattern(h, w, cn, seed=99):
    return np.random.default_rng(seed).integers(0, 256, (h, w, cn), dtype=np.uint8)


def _assert_device(R):
    kinds = R.last_launch_kinds()
    assert R.last_auto_radius_form() == "device", (R.last_auto_radius_form(), kinds)
    assert kinds and all(k in DEVICE_KINDS for k in kinds), kinds


def _oracle_pair(O, spec, imgs, r, size_in, out_wh, interp, border, bv, fill=None):
    xm, ym = O.get_map(spec, radius=r, size_input=size_in, size_output=out_wh)
    return [O.remap(im, xm, ym, interp, border, bv, dst=None if fill is None else fill.copy()) for im in imgs]


def _run_auto(R, dev, spec, srcs, out_wh, interp, border, bv, rad, fill, size_input=None):
    cn = int(srcs[0].shape[2])
    dsts = [torch.from_numpy(fill).to(dev) for _ in srcs]
    R.remap_tensors_auto(CS.to_product(spec), srcs, dsts, rad=rad, interpolation=interp, boarder_mode=border, boarder_value=bv,
                         size_input=size_input)
    assert dsts[0].shape == (out_wh[1], out_wh[0], cn)
    return [d.cpu().numpy() for d in dsts]


# ---------------------------------------------------------------------------------------------------------------------------------
# a. sampler x border x channels on the box-less launch, through both entry points
# ---------------------------------------------------------------------------------------------------------------------------------
def _exact_pair(V, R, spec, la, lb, fill, out_wh, interp, border):
    """apply_lr_tensors(auto_radius_on_device=True) where the device form declines: the exact form must serve it, from a planned
    launch (not the LUT path).  Returns the side-by-side result."""
    out = torch.from_numpy(np.concatenate([fill, fill], axis=1)).to(la.device)
    V.apply_lr_tensors(CS.to_product(spec), la, lb, out=out, size_output=out_wh, interpolation=interp, boarder_mode=border,
                       boarder_value=BV, radius="auto", auto_radius_on_device=True)
    kinds = R.last_launch_kinds()
    assert R.last_auto_radius_form() == "exact" and kinds and "lut" not in kinds, (R.last_auto_radius_form(), kinds)
    return out.cpu().numpy()


@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("border", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("interp", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("chain", ["rotated", "unrotated"])
def test_box_less_launch_sampler_border_channels(V, R, oracle_mod, dev, chain, interp, border, cn):
    """Two eyes of 384 x 448 (the centre row is get_radius's line), image circles of different radii, one of them off centre:
    the radius is the maximum of two negative estimates.  rad=None (the launch scans the sources itself) and rad=auto_radius_tensor
    (the two-step form) must give the oracle's bytes; TRANSPARENT keeps the pre-filled destination where the map leaves the source.
    Grayscale / BGRA: the device form needs a plan with one table entry per lane (k_ray_lin_cn's boxes) -- at these sources a
    1024-pixel output, not a 320-pixel one -- and dword-aligned sources; an unaligned view is declined and the exact form serves it,
    with the same bytes."""
    O = oracle_mod
    spec = SPEC_A if chain == "rotated" else SPEC_B
    h, w, out_wh = 384, 448, ((320, 320) if cn == 3 else (1024, 1024))
    imgs = [_disc(h, w, 181.5, 1, cn), _disc(h, w, 170, 2, cn, cx=w / 2 - 9)]
    r_ref = max(O.get_radius(im) for im in imgs)
    assert r_ref == -170.5
    fill = _pattern(out_wh[1], out_wh[0], cn)
    want = _oracle_pair(O, spec, imgs, r_ref, (h, w), out_wh, interp, border, BV, fill)
    srcs = [torch.from_numpy(im).to(dev) for im in imgs]
    for two_step in (False, True):
        rad = R.auto_radius_tensor(srcs) if two_step else None
        got = _run_auto(R, dev, spec, srcs, out_wh, interp, border, BV, rad, fill)
        _assert_device(R)
        if cn != 3:
            assert R.last_launch_kinds() == ["cn_rot"]
        for k in range(2):
            assert np.array_equal(got[k], want[k]), (two_step, k, r_ref, int((got[k] != want[k]).any(axis=2).sum()))
    if cn == 3:
        return
    # a view one byte into its buffer is declined (by both entry points) and served by the exact form
    views = []
    for im in imgs:
        buf = torch.zeros(h * (w + 1) * cn + 4, dtype=torch.uint8, device=dev)
        v = torch.as_strided(buf, (h, w, cn), ((w + 1) * cn, cn, 1), 1)
        v.copy_(torch.from_numpy(im).to(dev))
        assert v.data_ptr() % 4 == 1
        views.append(v)
    for rad in (None, R.auto_radius_tensor(views)):
        with pytest.raises(NotImplementedError, match="dword-aligned"):
            _run_auto(R, dev, spec, views, out_wh, interp, border, BV, rad, fill)
    assert np.array_equal(_exact_pair(V, R, spec, views[0], views[1], fill, out_wh, interp, border), np.concatenate(want, axis=1))


# ---------------------------------------------------------------------------------------------------------------------------------
# b. radius edges
# ---------------------------------------------------------------------------------------------------------------------------------
def _edge_pair(name):
    """(images, what the reference's radius is known to be) of one radius edge case"""
    if name == "two_negative":  # clean discs in both eyes
        return [_disc(400, 400, 190, 3), _disc(400, 400, 176.5, 4, cx=190)], lambda r: r < 0
    if name == "negative_and_positive":
        return [_disc(400, 400, 190, 5), _banded(400, 400, 6, [(60, 64), (330, 336)])], lambda r: r == (336 - 60) / 2
    if name == "equal":
        return [_banded(400, 400, 7, [(30, 40), (360, 372)]), _banded(400, 400, 8, [(30, 31), (371, 372)])], lambda r: r == 171.0
    if name == "half_integer":
        return [_banded(400, 400, 9, [(41, 50), (350, 360)]), _disc(400, 400, 150, 10)], lambda r: r == 159.5
    if name == "tiny_positive":  # one black pixel on the line: r = 0.5
        return [_banded(400, 400, 11, [(200, 201)]), _disc(400, 400, 170, 12)], lambda r: r == 0.5
    if name == "tiny_negative":  # one / two lit pixels on an otherwise black line: -0.5 and -1.5
        a, b = np.zeros((400, 400, 3), np.uint8), np.zeros((400, 400, 3), np.uint8)
        a[200], b[199:201] = 200, 90  # (rows: a square source's line is its centre column)
        return [b, a], lambda r: r == -0.5
    raise KeyError(name)


EDGES = ["two_negative", "negative_and_positive", "equal", "half_integer", "tiny_positive", "tiny_negative"]


@pytest.mark.parametrize("interp", [1, 4])
@pytest.mark.parametrize("name", EDGES)
def test_radius_edges(V, R, oracle_mod, dev, name, interp):
    O = oracle_mod
    imgs, pin = _edge_pair(name)
    r_ref = max(O.get_radius(im) for im in imgs)
    assert pin(r_ref), (name, r_ref)
    out_wh = (256, 256)
    fill = _pattern(256, 256, 3)
    want = _oracle_pair(O, SPEC_B, imgs, r_ref, imgs[0].shape[:2], out_wh, interp, 0, BV, fill)
    srcs = [torch.from_numpy(im).to(dev) for im in imgs]
    for rad in (None, R.auto_radius_tensor(srcs)):
        got = _run_auto(R, dev, SPEC_B, srcs, out_wh, interp, 0, BV, rad, fill)
        _assert_device(R)
        for k in range(2):
            assert np.array_equal(got[k], want[k]), (name, rad is None, k, r_ref)


@pytest.mark.parametrize("border", [0, 1, 2, 3, 4, 5])
def test_radius_beyond_the_short_side_of_a_landscape_source(V, R, oracle_mod, dev, border):
    """A 240 x 560 source whose centre row has black runs near both ends: |r| > src_h / 2, so the footprints leave the source above
    and below -- under every border mode, with the widest sampler."""
    O = oracle_mod
    h, w = 240, 560
    imgs = [_banded(h, w, 13, [(6, 11), (548, 553)]), _banded(h, w, 14, [(20, 24), (530, 540)])]
    r_ref = max(O.get_radius(im) for im in imgs)
    assert r_ref == (553 - 6) / 2 and r_ref > h / 2
    out_wh = (288, 288)
    fill = _pattern(288, 288, 3)
    for interp in (4, 1):
        want = _oracle_pair(O, SPEC_A, imgs, r_ref, (h, w), out_wh, interp, border, BV, fill)
        srcs = [torch.from_numpy(im).to(dev) for im in imgs]
        for rad in (None, R.auto_radius_tensor(srcs)):
            got = _run_auto(R, dev, SPEC_A, srcs, out_wh, interp, border, BV, rad, fill)
            _assert_device(R)
            for k in range(2):
                assert np.array_equal(got[k], want[k]), (interp, rad is None, k, int((got[k] != want[k]).any(axis=2).sum()))


@pytest.mark.parametrize("border", [0, 3])
def test_explicit_radius_at_and_beyond_the_clamp(V, R, oracle_mod, dev, border):
    """rad = exactly +-4 max(src_h, src_w) is taken as is; beyond it the header's clamp holds: the output equals the oracle's at the
    clamped radius.  A rad tensor with more rows than units: the maximum over every row."""
    O = oracle_mod
    h, w = 200, 232
    lim = 4.0 * max(h, w)
    imgs = [_disc(h, w, 90, 15), _disc(h, w, 95, 16)]
    srcs = [torch.from_numpy(im).to(dev) for im in imgs]
    out_wh = (224, 224)
    fill = _pattern(224, 224, 3)
    cases = [([lim], lim), ([-lim], -lim), ([lim * 1.5, 3.0], lim), ([-lim - 0.5], -lim), ([-5 * lim, -lim - 7], -lim),
             ([40.0, -3.0, 97.5, 12.0], 97.5), ([-60.0, -61.0, -59.5], -59.5)]
    for rows, r_used in cases:
        rad = torch.tensor([[r, 0.0] for r in rows], dtype=torch.float64, device=dev)
        want = _oracle_pair(O, SPEC_B, imgs, r_used, (h, w), out_wh, 4, border, BV, fill)
        got = _run_auto(R, dev, SPEC_B, srcs, out_wh, 4, border, BV, rad, fill)
        _assert_device(R)
        for k in range(2):
            assert np.array_equal(got[k], want[k]), (rows, k)


# ---------------------------------------------------------------------------------------------------------------------------------
# c. chains through apply_lr_tensors(radius="auto")
# ---------------------------------------------------------------------------------------------------------------------------------
_PLANAR = list(CS.PLANAR_CASES)[:3]
CHAINS = {  # name: (spec or per-eye tuple of specs, the device form serves it)
    **{f"dec_{m}": ([("equirect_enc", True), ("fisheye_dec", m)], m != "rectilinear") for m in
       ("rectilinear", "stereographic", "equidistant", "equisolid", "orthographic")},
    "rot_quat": ([("equirect_enc", True), ("rot_quat", CS.rotvec_quat([0.1, -0.25, 0.05])), CS.EQUI], True),
    "poly_c0": ([("equirect_enc", True), ("poly", [0.05, 1, -0.1]), CS.EQUI], False),  # needs a fix-up pass
    **{f"planar_{k}": (CS.PLANAR_CASES[k][0], False) for k in _PLANAR},
    "per_eye": (([("equirect_enc", True), ("rot", CS.ry(0.05)), CS.EQUI], SPEC_B), True),
}


def _product(spec):
    return tuple(CS.to_product(s) for s in spec) if isinstance(spec, tuple) else CS.to_product(spec)


@pytest.mark.parametrize("on_device", [None, False, True])
@pytest.mark.parametrize("name", list(CHAINS))
def test_chains_through_apply_lr_tensors(V, R, oracle_mod, dev, name, on_device):
    O = oracle_mod
    spec, device_serves = CHAINS[name]
    a, b = _disc(360, 360, 170, 17), _disc(360, 360, 158.5, 18, cx=176)
    t = _product(spec)
    got = V.apply_lr_tensors(t, torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), size_output=(288, 288), interpolation=4,
                             boarder_value=BV, radius="auto", auto_radius_on_device=on_device)
    kinds = R.last_launch_kinds()
    if on_device and device_serves:
        _assert_device(R)
    else:
        assert R.last_auto_radius_form() == "exact" and kinds and "lut" not in kinds, (R.last_auto_radius_form(), kinds)
    want = O.apply_lr(spec, a, b, size_output=(288, 288), interpolation=4, border_value=BV, radius="auto")
    assert np.array_equal(got.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------------------------
# d. the two regressions of the device form: chains that cannot be lowered, eyes of different shapes
# ---------------------------------------------------------------------------------------------------------------------------------
NOT_LOWERABLE = {
    "poly17": [("equirect_enc", True), ("poly", [0.0, 1.0] + [0.0] * 14 + [-0.01]), CS.EQUI],
    "stages17": [("equirect_enc", True)] + [("zoom", 1.0 + 0.001 * k) for k in range(1, 15)] + [CS.EQUI],
}


@pytest.mark.parametrize("on_device", [None, False, True])
@pytest.mark.parametrize("name", list(NOT_LOWERABLE))
def test_auto_radius_of_a_chain_that_cannot_be_lowered(V, R, oracle_mod, dev, name, on_device):
    """remap_tensors_auto raised chain.NotLowerable, which neither caller caught: the default apply_lr_tensors(t, L, R) failed.  Now the
    LUT path serves it, with the map of the chain's own transform() -- the oracle's NumPy evaluation, float32."""
    from oracle import chain_numpy

    O = oracle_mod
    spec = NOT_LOWERABLE[name]
    a, b = _disc(320, 320, 150, 19), _disc(320, 320, 141, 20)
    r_ref = max(O.get_radius(a), O.get_radius(b))
    xw, yw = chain_numpy.get_map(spec, radius=r_ref, size_input=(320, 320), size_output=(256, 256))
    xw, yw = xw.astype(np.float32), yw.astype(np.float32)
    xm, ym = V.get_map(CS.to_product(spec), radius=r_ref, size_input=(320, 320), size_output=(256, 256))
    assert np.array_equal(xm, xw) and np.array_equal(ym, yw)
    got = V.apply_lr_tensors(CS.to_product(spec), torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), size_output=(256, 256),
                             interpolation=1, radius="auto", auto_radius_on_device=on_device)
    assert R.last_auto_radius_form() == "exact" and R.last_launch_kinds() == ["lut", "lut"], R.last_launch_kinds()
    want = np.concatenate([O.remap(im, xw, yw, 1, 0, 0) for im in (a, b)], axis=1)
    assert np.array_equal(got.cpu().numpy(), want)


def _uneven_pairs(dev):
    """(name, left view, right view, left array, right array): the halves of an odd-width side-by-side frame, and eyes of different
    heights"""
    frame = np.concatenate([_disc(300, 300, 140, 21), _disc(300, 301, 136.5, 22)], axis=1)  # W = 601
    f = torch.from_numpy(frame).to(dev)
    yield "odd_width_sbs", f[:, :300], f[:, 300:], frame[:, :300], frame[:, 300:]
    a, b = _disc(300, 320, 139, 23), _disc(340, 320, 150, 24)
    yield "different_heights", torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), a, b


@pytest.mark.parametrize("interp", [1, 4])
def test_auto_radius_of_eyes_of_different_shapes(V, R, oracle_mod, dev, interp):
    """One shared transformer over eyes of different shapes: one plan was made from srcs[0].shape and marshal_units refused the other
    eye (ValueError) in both forms.  Now: one radius over both sources, one launch per shape, images[0]'s centre (remapper.py:385) --
    what the oracle's apply_lr does."""
    O = oracle_mod
    t = CS.to_product(SPEC_A)
    for name, la, lb, a, b in _uneven_pairs(dev):
        want = O.apply_lr(SPEC_A, a, b, size_output=(256, 256), interpolation=interp, border_value=BV, radius="auto")
        for on_device in (None, False, True):
            got = V.apply_lr_tensors(t, la, lb, size_output=(256, 256), interpolation=interp, boarder_value=BV, radius="auto",
                                     auto_radius_on_device=on_device)
            if on_device:
                _assert_device(R)
                assert len(R.last_launch_kinds()) == 2
            else:
                assert R.last_auto_radius_form() == "exact" and R.last_launch_kinds(), R.last_launch_kinds()
            assert np.array_equal(got.cpu().numpy(), want), (name, on_device)


def test_auto_radius_of_eyes_of_different_shapes_in_a_graph(V, R, oracle_mod, dev):
    """The same call recorded into a graph (the device form by itself: capturing) and replayed on new pixels with other circles."""
    O = oracle_mod
    t = CS.to_product(SPEC_A)
    frames = [np.concatenate([_disc(300, 300, r0, 25 + k), _disc(300, 301, r1, 35 + k)], axis=1)
              for k, (r0, r1) in enumerate(((140, 136.5), (121, 144), (133.5, 118)))]
    f = torch.from_numpy(frames[0]).to(dev)
    out = torch.zeros((256, 512, 3), dtype=torch.uint8, device=dev)
    V.apply_lr_tensors(t, f[:, :300], f[:, 300:], out=out, size_output=(256, 256), radius="auto", auto_radius_on_device=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream(device=dev)):
        V.apply_lr_tensors(t, f[:, :300], f[:, 300:], out=out, size_output=(256, 256), radius="auto")
    assert R.last_auto_radius_form() == "device"
    for fr in frames[::-1]:
        f.copy_(torch.from_numpy(fr).to(dev))
        out.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = O.apply_lr(SPEC_A, fr[:, :300], fr[:, 300:], size_output=(256, 256), interpolation=4, radius="auto")
        assert np.array_equal(out.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------------------------
# e. no black border on the device form
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", [0, 1, 2, 3, 4, 5])
def test_no_black_border_on_the_device(V, R, oracle_mod, dev, border):
    """The reference raises IndexError; the device form sets scale 0 and the centre (-40000, -40000): every output pixel samples there
    under the border mode (include/vr180_remap.h, v1c_plan_run_auto) -- the border colour, the untouched destination, or what
    REPLICATE / REFLECT / WRAP / REFLECT_101 read at that point."""
    O = oracle_mod
    full = np.random.default_rng(26).integers(40, 256, (240, 250, 3), dtype=np.uint8)
    disc = _disc(240, 250, 110, 27)
    with pytest.raises(IndexError):
        O.get_radius(full)
    far = np.full((192, 192), -40000.0, np.float32)
    fill = _pattern(192, 192, 3)
    srcs = [torch.from_numpy(full).to(dev), torch.from_numpy(disc).to(dev)]
    for interp in (1, 4):
        for rad in (None, R.auto_radius_tensor(srcs)):
            got = _run_auto(R, dev, SPEC_B, srcs, (192, 192), interp, border, BV, rad, fill)
            _assert_device(R)
            for k, im in enumerate((full, disc)):
                want = O.remap(im, far, far, interp, border, BV, dst=fill.copy())
                assert np.array_equal(got[k], want), (interp, rad is None, k)
    if border == 0:
        assert np.array_equal(got[0], np.broadcast_to(np.array(BV[:3], np.uint8), got[0].shape))
    if border == 5:
        assert np.array_equal(got[0], fill)


# ---------------------------------------------------------------------------------------------------------------------------------
# f. C ABI: an anisotropic Denormalize is refused
# ---------------------------------------------------------------------------------------------------------------------------------
def test_run_auto_refuses_an_anisotropic_denormalize(V, R, dev):
    """The launch writes the scale (r, r): a plan built through the ABI with rx != ry must get V1C_E_UNSUPPORTED from
    v1c_plan_run_auto (both forms), before anything is launched -- the destination keeps its bytes."""
    from vr180_convert_amd import _abi, _native
    from vr180_convert_amd.chain import lower_for_get_map

    ch = lower_for_get_map(CS.to_product(SPEC_B), radius=100.0, size_input=(200, 200), size_output=(128, 128))
    den = [i for i in range(ch.n_ops) if ch.ops[i].opcode == _abi.OP_DENORMALIZE]
    assert len(den) == 1
    plan_iso = R.Plan(ch, src_hw=(200, 200), dst_wh=(128, 128), cn=3, interpolation=1, border_mode=0, border_value=0, device=dev)
    ch.ops[den[0]].p[1] = 80.0  # ry != rx
    plan = R.Plan(ch, src_hw=(200, 200), dst_wh=(128, 128), cn=3, interpolation=1, border_mode=0, border_value=0, device=dev)
    src = torch.from_numpy(_disc(200, 200, 90, 28)).to(dev)
    fill = torch.from_numpy(_pattern(128, 128, 3)).to(dev)
    dst = fill.clone()
    units = R.marshal_units([src], [dst], None, src_hw=(200, 200), dst_wh=(128, 128), cn=3, device=dev)
    rad = torch.tensor([[90.0, 0.0]], dtype=torch.float64, device=dev)
    lib = _native.lib()
    stream = R._stream_ptr(dev)
    assert lib.v1c_plan_run_auto(plan._h, stream, units, 1, rad.data_ptr(), 1) == _abi.E_UNSUPPORTED
    assert b"isotropic" in lib.v1c_last_error()
    assert lib.v1c_plan_run_auto_images(plan._h, stream, units, 1, 10) == _abi.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(dst, fill)
    # (the same chain with rx == ry is served)
    assert lib.v1c_plan_run_auto(plan_iso._h, stream, units, 1, rad.data_ptr(), 1) == _abi.OK
    torch.cuda.synchronize()
    assert not torch.equal(dst, fill)
