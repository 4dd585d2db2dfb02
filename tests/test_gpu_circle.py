"""The image-circle fit on the device: every case of tests/circle_cases.py through ``v1c_fit_circle`` against
the restatement -- rim points, selection flags and counts equal, floats within 1e-9 px --, ``fit_circle_tensor`` under graph capture and
from two threads, and the remap entry points with ``center=`` and ``radius="fit"`` byte for byte against the oracle's remap of the host
NumPy chain's map with that centre."""
import functools
import threading

import numpy as np
import pytest
import torch

import circle_cases as CC

pytestmark = pytest.mark.gpu

NAMES = sorted(CC.shared_cases())


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _view(case, dev):
    """the case's view of its base array, on the device: the same pitch and the same odd offsets as on the host"""
    return torch.from_numpy(case.base).to(dev)[case.view]


def same_fit(got, want, what=""):
    (out, rim), (wout, wrim) = got, want
    assert np.array_equal(rim, wrim), what
    assert list(out[3:6]) == list(wout[3:6]) and out[7] == 0, (what, out, wout)
    assert np.abs(out[[0, 1, 2, 6]] - wout[[0, 1, 2, 6]]).max() <= 1e-9, (what, out, wout)


def test_every_case_equals_the_restatement(dev):
    from vr180_convert_amd import circle

    for name in NAMES:
        case = CC.shared_cases()[name]
        t = _view(case, dev)
        assert t.is_contiguous() == case.img.flags.c_contiguous
        got = circle.fit_circle_raw(t, points=True, **case.kw)
        same_fit(got, CC.reference(name), name)
        again = circle.fit_circle_raw(t, points=True, **case.kw)
        assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]), name  # two calls, the same eight doubles


def test_fit_circle_and_its_errors(dev):
    import vr180_convert_amd as V

    case = CC.shared_cases()["aa_disc_1"]
    c = V.fit_circle(case.img, device=dev)  # a numpy image goes up
    want = CC.reference("aa_disc_1")[0]
    assert isinstance(c, V.Circle) and abs(c.cx - want[0]) <= 1e-9 and abs(c.cy - want[1]) <= 1e-9 and abs(c.radius - want[2]) <= 1e-9
    assert (c.n_rim, c.n_used) == (int(want[4]), int(want[5])) and c.radius > 0
    for name in ("all_black", "all_lit", "one_lit_pixel"):
        with pytest.raises(ValueError, match="no image circle found"):
            V.fit_circle(_view(CC.shared_cases()[name], dev))
    with pytest.raises(TypeError):
        V.fit_circle_tensor(torch.zeros((8, 8, 3), dtype=torch.float32, device=dev))
    with pytest.raises(TypeError):
        V.fit_circle(np.zeros((8, 8, 3), np.float32), device=dev)


def test_fit_circle_tensor_under_graph_capture_replayed_on_a_changed_image(dev):
    import vr180_convert_amd as V

    a, b = CC.shared_cases()["aa_disc_1"], CC.shared_cases()["aa_disc_2"]
    assert a.img.shape == b.img.shape
    buf = torch.from_numpy(np.ascontiguousarray(a.img)).to(dev)
    V.fit_circle_tensor(buf)  # (the library is loaded and the kernels are resident before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = V.fit_circle_tensor(buf)
    for case, name in ((a, "aa_disc_1"), (b, "aa_disc_2"), (a, "aa_disc_1")):
        buf.copy_(torch.from_numpy(np.ascontiguousarray(case.img)).to(dev))
        g.replay()
        torch.cuda.synchronize()
        got, want = out.cpu().numpy(), CC.reference(name)[0]
        assert list(got[3:6]) == list(want[3:6]) and np.abs(got - want).max() <= 1e-9, (name, got, want)


def test_two_threads_on_streams_of_their_own(dev):
    import vr180_convert_amd as V

    names = [n for n in NAMES if CC.shared_cases()[n].truth is not None]
    imgs = {n: _view(CC.shared_cases()[n], dev) for n in names}
    V.fit_circle_tensor(imgs[names[0]])
    torch.cuda.synchronize()
    errors: list = []

    def work(order):
        try:
            s = torch.cuda.Stream(dev)
            with torch.cuda.stream(s):
                outs = [(n, V.fit_circle_tensor(imgs[n], **CC.shared_cases()[n].kw)) for n in order]
                s.synchronize()
            for n, o in outs:
                got, want = o.cpu().numpy(), CC.reference(n)[0]
                assert list(got[3:6]) == list(want[3:6]) and np.abs(got - want).max() <= 1e-9, (n, got, want)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=work, args=(names,)), threading.Thread(target=work, args=(names[::-1],))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


# ---- the remap entry points with center= and radius="fit" ------------------------------------------------------------------------------
INTERPOLATIONS = {"nearest": 0, "bilinear": 1, "lanczos4": 4}
SIZES = {"small": ((80, 96), (64, 64)), "tiled": ((512, 640), (512, 512))}  # (source (H, W), result (W, H))
TILED_KINDS = ("tile", "mirror", "batch", "rot_pair", "cn")


def _chain():
    import vr180_convert_amd as V

    return V.EquirectangularEncoder() * V.FisheyeDecoder("equidistant")


@functools.lru_cache(maxsize=None)
def _eyes(size):
    """two noise discs off the frame's centre (every lit pixel >= 40: a sharp rim), their centres on the 1/4 px grid and their radius"""
    (h, w), _ = SIZES[size]
    r = 0.36 * h
    cl, cr = (0.55 * w - 0.05, 0.47 * h + 0.15), (0.46 * w + 0.2, 0.52 * h - 0.1)
    rng = np.random.default_rng(11)
    out = []
    for cx, cy in (cl, cr):
        a = rng.integers(40, 256, (h, w, 3), dtype=np.uint8)
        a[CC.disc(h, w, cx, cy, r, aa=False)[..., 0] == 0] = 0
        a.setflags(write=False)
        out.append(a)
    return out[0], out[1], r


@functools.lru_cache(maxsize=None)
def _fitted(size):
    """what center="auto" and radius="fit" resolve to, by the restatement: centres on the 1/4 px grid, the larger radius on the 1/2 px one"""
    import circle_ref as R
    from vr180_convert_amd import circle

    fits = [R.fit(im)[0] for im in _eyes(size)[:2]]
    assert all(f[3] == 0 for f in fits)
    return [circle.round_center(f[0], f[1]) for f in fits], max(circle.round_radius(f[2]) for f in fits)


@functools.lru_cache(maxsize=None)
def _want(size, interp, center, radius, eye):
    """oracle.remap of the host NumPy chain's map with that centre; computed once per configuration"""
    from oracle import oracle as O
    from vr180_convert_amd import remapper

    O.build()
    size_in, size_out = SIZES[size]
    xm, ym = remapper._host_map(_chain(), radius=radius, size_input=size_in, size_output=size_out, center=center)
    out = O.remap(_eyes(size)[eye], xm, ym, INTERPOLATIONS[interp])
    out.setflags(write=False)
    return out


def _check(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    bad = int((got != want).sum())
    print(f"{what}: {bad} of {want.size} bytes differ")
    assert got.shape == want.shape and bad == 0, what


@pytest.mark.parametrize("interp", sorted(INTERPOLATIONS))
@pytest.mark.parametrize("size", sorted(SIZES))
def test_apply_and_apply_lr_with_centres_equal_the_oracle(dev, size, interp):
    import vr180_convert_amd as V
    from vr180_convert_amd import remapper

    left, right, r = _eyes(size)
    size_out = SIZES[size][1]
    (h, w) = SIZES[size][0]
    kw = dict(size_output=size_out, interpolation=INTERPOLATIONS[interp])
    cl, cr = (0.55 * w - 0.25, 0.47 * h + 0.25), (0.46 * w + 0.25, 0.52 * h)
    kinds = {}
    # one explicit off-centre centre for every image
    got = V.apply(_chain(), in_paths=[left, right], radius=r, center=cl, device=dev, **kw)
    kinds["apply explicit"] = remapper.last_launch_kinds()
    for eye in (0, 1):
        _check(got[eye], _want(size, interp, cl, r, eye), f"apply explicit eye {eye}")
    # a centre per image
    got = V.apply(_chain(), in_paths=[left, right], radius=r, center=[cl, cr], device=dev, **kw)
    kinds["apply per image"] = remapper.last_launch_kinds()
    for eye, c in enumerate((cl, cr)):
        _check(got[eye], _want(size, interp, c, r, eye), f"apply per-image eye {eye}")
    lt, rt = torch.from_numpy(left.copy()).to(dev), torch.from_numpy(right.copy()).to(dev)
    wo = size_out[0]
    sbs = V.apply_lr_tensors(_chain(), lt, rt, radius=r, center=cl, **kw)
    kinds["apply_lr explicit"] = remapper.last_launch_kinds()
    _check(sbs[:, :wo], _want(size, interp, cl, r, 0), "apply_lr explicit left")
    _check(sbs[:, wo:], _want(size, interp, cl, r, 1), "apply_lr explicit right")
    sbs = V.apply_lr_tensors(_chain(), lt, rt, radius=r, center=(cl, cr), **kw)
    kinds["apply_lr per eye"] = remapper.last_launch_kinds()
    _check(sbs[:, :wo], _want(size, interp, cl, r, 0), "apply_lr per-eye left")
    _check(sbs[:, wo:], _want(size, interp, cr, r, 1), "apply_lr per-eye right")
    # fitted centres, each eye its own, and the fitted radius
    (fl, fr), rf = _fitted(size)
    assert fl != fr and abs(fl[0] - (0.55 * w - 0.05)) <= 0.25 and abs(fr[1] - (0.52 * h - 0.1)) <= 0.25 and abs(rf - r) <= 1.0
    sbs = V.apply_lr_tensors(_chain(), lt, rt, radius="fit", center="auto", **kw)
    kinds["apply_lr auto"] = remapper.last_launch_kinds()
    _check(sbs[:, :wo], _want(size, interp, fl, rf, 0), "apply_lr auto left")
    _check(sbs[:, wo:], _want(size, interp, fr, rf, 1), "apply_lr auto right")
    got = V.apply(_chain(), in_paths=[left, right], radius="fit", center="auto", device=dev, **kw)
    for eye, c in enumerate((fl, fr)):
        _check(got[eye], _want(size, interp, c, rf, eye), f"apply auto eye {eye}")
    print(size, interp, kinds)
    if size == "tiled":
        # an off-centre chain is served by the tiled kernels, not by the fp64 interpreter or the LUT path
        for what, ks in kinds.items():
            assert ks and all(k.split("+")[0] in TILED_KINDS for k in ks), (what, ks)


def test_apply_lr_writes_one_side_by_side_file_fitted_per_half(dev, tmp_path):
    """one file holding both eyes: each half is fitted in its own coordinates -- the case center="auto" exists for"""
    import vr180_convert_amd as V
    from vr180_convert_amd import _io

    left, right, r = _eyes("small")
    src = tmp_path / "sbs.png"
    _io.imwrite(src, np.concatenate([left, right], axis=1))
    out = tmp_path / "out.png"
    V.apply_lr(_chain(), left_path=src, right_path=src, out_path=out, size_output=(64, 64), interpolation=1, radius="fit", center="auto", device=dev)
    got = np.asarray(_io.imread(out))
    (fl, fr), rf = _fitted("small")
    _check(got[:, :64], _want("small", "bilinear", fl, rf, 0), "sbs file left")
    _check(got[:, 64:], _want("small", "bilinear", fr, rf, 1), "sbs file right")


def test_explicit_centres_under_capture_and_with_the_device_resident_radius(dev):
    """explicit centres work where center="auto" is refused: auto_radius_on_device=True and a captured stream"""
    import vr180_convert_amd as V
    from oracle import oracle as O
    from vr180_convert_amd import remapper

    left, right, _ = _eyes("small")
    lt, rt = torch.from_numpy(left.copy()).to(dev), torch.from_numpy(right.copy()).to(dev)
    cl, cr = (52.5, 37.75), (44.5, 41.5)
    r_auto = max(O.get_radius(left), O.get_radius(right))  # radius="auto" keeps its value, sign included
    kw = dict(size_output=(64, 64), interpolation=1)
    for center, cs in ((cl, (cl, cl)), ((cl, cr), (cl, cr))):
        sbs = V.apply_lr_tensors(_chain(), lt, rt, radius="auto", auto_radius_on_device=True, center=center, **kw)
        assert remapper.last_auto_radius_form() == "device"
        _check(sbs[:, :64], _want("small", "bilinear", cs[0], r_auto, 0), "device radius left")
        _check(sbs[:, 64:], _want("small", "bilinear", cs[1], r_auto, 1), "device radius right")
        exact = V.apply_lr_tensors(_chain(), lt, rt, radius="auto", auto_radius_on_device=False, center=center, **kw)
        assert torch.equal(exact, sbs)
    with pytest.raises(NotImplementedError):
        V.apply_lr_tensors(_chain(), lt, rt, radius="auto", auto_radius_on_device=True, center="auto", **kw)
    out = torch.zeros((64, 128, 3), dtype=torch.uint8, device=dev)
    V.apply_lr_tensors(_chain(), lt, rt, out=out, radius=30.0, center=(cl, cr), **kw)  # (the plans exist before the capture)
    want = out.clone()
    out.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        V.apply_lr_tensors(_chain(), lt, rt, out=out, radius=30.0, center=(cl, cr), **kw)
        with pytest.raises(NotImplementedError):
            V.apply_lr_tensors(_chain(), lt, rt, out=out, radius=30.0, center="auto", **kw)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    _check(out[:, 64:], _want("small", "bilinear", cr, 30.0, 1), "captured right")


def test_radius_fit_on_a_clipped_circle_where_auto_raises(dev):
    import vr180_convert_amd as V
    from vr180_convert_amd import remapper

    case = CC.shared_cases()["clip_4"]  # clipped on four sides: no black border on the centre row
    img = np.ascontiguousarray(case.img)
    with pytest.raises(IndexError):
        V.apply(_chain(), in_paths=[img], radius="auto", size_output=(64, 64), interpolation=1, device=dev)
    t = torch.from_numpy(img).to(dev)
    with pytest.raises(IndexError):
        remapper.get_radius_smart("auto", [t])
    want = CC.reference("clip_4")[0]
    r = remapper.get_radius_smart("fit", [t])
    assert r > 0 and r == np.floor(want[2] * 2 + 0.5) / 2 and abs(r - 50) <= 0.5
    got = V.apply(_chain(), in_paths=[img], radius="fit", center="auto", size_output=(64, 64), interpolation=1, device=dev)
    from oracle import oracle as O

    c = (float(np.floor(want[0] * 4 + 0.5) / 4), float(np.floor(want[1] * 4 + 0.5) / 4))
    xm, ym = remapper._host_map(_chain(), radius=r, size_input=(80, 96), size_output=(64, 64), center=c)
    _check(got[0], O.remap(img, xm, ym, 1), "clipped circle")
