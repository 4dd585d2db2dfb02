"""The image-circle fit without a device: the restatement (tests/circle_ref.py) against a host build of
circle_core.hpp driven through the kernels' decomposition (tests/host_circle/circle_emul.hip), the same program under the address and
undefined-behaviour sanitizers, the accuracy of the fit on discs with a known centre and on the reference's docs photo, the argument
checks of the C ABI, and the Python plumbing of ``center=`` and ``radius="fit"`` with the device monkeypatched away."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import circle_cases as CC
import circle_ref as R

ROOT = Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "host_circle" / "circle_emul.hip"
NAMES = sorted(CC.shared_cases())


def _prm(kw):
    d = dict(R.DEFAULTS, **kw)
    tol = list(d["tol16"]) + [24] * 8
    return [d["threshold"], d["run"], d["rounds"], d["min_points"]] + [tol[k] if k < d["rounds"] else 0 for k in range(8)]


@pytest.fixture(scope="module")
def circle_emul(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_circle") / "libcircle_emul.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-fno-fast-math", "-o", str(out),
                    str(HARNESS)], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(out))
    lib.circle_emul_fit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def _emul(lib, img, kw):
    a = img if img.ndim == 3 else img[..., None]
    h, w, cn = a.shape
    assert a.strides[2] == a.itemsize and a.strides[1] == cn * a.itemsize
    prm = np.array(_prm(kw), np.int32)
    out = np.zeros(8, np.float64)
    pts = np.zeros((2 * (h + w), 3), np.int32)
    n = lib.circle_emul_fit(a.ctypes.data, h, w, a.strides[0], cn, int(a.dtype == np.uint16), prm.ctypes.data, out.ctypes.data, pts.ctypes.data)
    return out, pts[:n]


def same_fit(got, want):
    """integers equal, floats within 1e-9 px (the issue's bound: anything more means two different operation sequences)"""
    (out, rim), (wout, wrim) = got, want
    assert np.array_equal(rim, wrim)
    assert list(out[3:6]) == list(wout[3:6]) and out[7] == wout[7] == 0
    assert np.abs(out[[0, 1, 2, 6]] - wout[[0, 1, 2, 6]]).max() <= 1e-9, (out, wout)


@pytest.mark.parametrize("name", NAMES)
def test_product_host_code_equals_restatement(circle_emul, name):
    case = CC.shared_cases()[name]
    same_fit(_emul(circle_emul, case.img, case.kw), CC.reference(name))


def test_the_cases_cover_what_they_are_meant_to():
    """a case table that never reaches a status, a dropped point or a trimmed point checks less than it says"""
    refs = {n: CC.reference(n) for n in NAMES}
    status = {n: int(o[3]) for n, (o, _) in refs.items()}
    assert {0, 1, 2} <= set(status.values())
    assert status["all_black"] == status["all_lit"] == status["one_lit_pixel"] == status["alpha_just_below"] == 1
    assert refs["all_lit"][0][4] == 0  # every point of an all-lit frame lies on the frame
    assert status["wedge"] == status["hot_pixels"] == 0
    assert refs["wedge"][0][5] < refs["wedge"][0][4]  # trimmed
    assert len(refs["one_lit_pixel_run_1"][1]) == 4
    for s in (61, 62, 63):
        rim = refs[f"row_cross_left_{s}"][1]
        assert (s, 1) in {(int(x), int(y)) for x, y, _ in rim} and (100, 3) in {(int(x), int(y)) for x, y, _ in rim}
        rim = refs[f"col_cross_top_{s}"][1]
        assert (1, s) in {(int(x), int(y)) for x, y, _ in rim} and (3, 100) in {(int(x), int(y)) for x, y, _ in rim}
    # (+ 2: the scans across find that line's two ends, which do not lie on THEIR frame edge)
    for x, kept in ((0, 0), (1, 14), (98, 14), (99, 0)):
        assert sum(1 for px, _, _ in refs[f"rim_col_{x}"][1] if px == x) == kept + 2
    for y, kept in ((0, 0), (1, 24), (38, 24), (39, 0)):
        assert sum(1 for _, py, _ in refs[f"rim_row_{y}"][1] if py == y) == kept + 2
    assert refs["threshold_65535_u8"][0][4] == 0 and refs["threshold_65535_u16"][0][3] == 0 and refs["threshold_0"][0][4] == 0


def test_known_truth_centres():
    """the restatement's centre within 0.125 px of the truth: half the 1/4 px grid the entry points round fitted centres to"""
    for name, case in CC.shared_cases().items():
        if case.truth is None:
            continue
        out, _ = CC.reference(name)
        assert out[3] == 0, name
        err = max(abs(out[0] - case.truth[0]), abs(out[1] - case.truth[1]))
        print(f"{name}: centre error {err:.4f} px, r {out[2]:.3f}, used {int(out[5])} of {int(out[4])}, rms {out[6]:.3f}")
        assert err <= 0.125, (name, out)


@pytest.fixture(scope="module")
def photo_cases():
    """the reference's docs photo (its circle touches the 2048 x 2048 frame), pasted into a black 2560 x 2304 frame at (317, 100), with a
    dark 300 x 80 patch on the centre row's left rim, and with 400 white pixels scattered in the border"""
    from vr180_convert_amd import _io

    img = np.asarray(_io.imread_many([str(ROOT / "tests" / "golden" / "ref_docs" / "test.jpg")])[0])
    assert img.shape == (2048, 2048, 3)

    def pasted():
        f = np.zeros((2304, 2560, 3), np.uint8)
        f[100:2148, 317:2365] = img
        return f

    wedge = pasted()
    wedge[1124 - 40:1124 + 40, 305:605] = 0
    hot = pasted()
    rng = np.random.default_rng(5)
    k = 0
    for y, x in zip(rng.integers(0, 2304, 4000), rng.integers(0, 2560, 4000)):
        if (x - 1341) ** 2 + (y - 1124) ** 2 > 1060 ** 2 and k < 400:
            hot[y, x] = 255
            k += 1
    assert k == 400
    return {"docs": img, "pasted": pasted(), "wedge": wedge, "hot": hot}


def test_photo_centres_and_radii(photo_cases, circle_emul):
    fits = {n: R.fit(im) for n, im in photo_cases.items()}
    for n, (out, _) in fits.items():
        print(n, [round(float(v), 4) for v in out])
        assert out[3] == 0
    for n in ("pasted", "wedge", "hot"):
        out = fits[n][0]
        assert abs(out[0] - 1341) <= 0.125 and abs(out[1] - 1124) <= 0.125, (n, out)
        assert abs(out[2] - fits["docs"][0][2]) <= 0.125 and abs(out[2] - fits["pasted"][0][2]) <= 0.125, (n, out)
    assert abs(fits["docs"][0][0] - 1024) <= 0.125 and abs(fits["docs"][0][1] - 1024) <= 0.125
    # the estimator the fit replaces, on the same frames: a chord, a shorter chord, IndexError
    from vr180_convert_amd.chain import get_radius

    assert get_radius(photo_cases["pasted"]) == 1018.5 and get_radius(photo_cases["wedge"]) < 900
    with pytest.raises(IndexError):
        get_radius(photo_cases["docs"])
    # and the product's host code on the full-size frames
    for n in ("docs", "wedge"):
        same_fit(_emul(circle_emul, photo_cases[n], {}), fits[n])


def test_sanitized_program_over_the_cases(tmp_path):
    """the harness as a program of its own under the address and undefined-behaviour sanitizers: every case from a heap copy of the
    exact size of its base array; any report fails the run, and what it prints is the restatement's"""
    exe = tmp_path / "circle_san"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fno-fast-math", "-DCIRCLE_MAIN", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(HARNESS)], check=True,
                   capture_output=True, timeout=600)
    lines = []
    for k, name in enumerate(NAMES):
        case = CC.shared_cases()[name]
        img = case.img
        p = tmp_path / f"case_{k}.raw"
        p.write_bytes(case.base.tobytes())
        offset = img.__array_interface__["data"][0] - case.base.__array_interface__["data"][0]
        lines.append(" ".join(str(v) for v in [img.shape[0], img.shape[1], img.strides[0], img.shape[2], int(img.dtype == np.uint16), offset,
                                               *_prm(case.kw), p]))
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(tmp_path / "list.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    rows = r.stdout.strip().split("\n")
    assert len(rows) == len(NAMES)
    for name, row in zip(NAMES, rows):
        f = row.split()
        out = np.array([float.fromhex(v) for v in f[:8]])
        n = int(f[8])
        rim = np.array([int(v) for v in f[9:]], np.int32).reshape(n, 3)
        same_fit((out, rim), CC.reference(name))


# ---- the C ABI's argument checks: before any device call -------------------------------------------------------------------------------
class Params(C.Structure):
    _fields_ = [("threshold", C.c_int32), ("run", C.c_int32), ("rounds", C.c_int32), ("min_points", C.c_int32), ("tol16", C.c_int32 * 8)]


def test_workspace_size(product_lib):
    ws = product_lib.v1c_fit_circle_workspace
    assert ws(0, 5) == ws(5, 0) == ws(32769, 5) == 0
    for h, w in ((1, 1), (65, 257), (4096, 8192), (32768, 32768)):
        n = 2 * (h + w)
        assert ws(h, w) == -(-4 * n // 256) * 256 + -(-n // 256) * 256 + 256 + -(-(-(-h // 64) * w * 4) // 256) * 256  # (+ the band records)


def test_argument_errors_come_before_any_device_call(product_lib):
    from vr180_convert_amd import _abi

    L = product_lib
    buf = np.zeros(4096, np.uint8)
    p, out = buf.ctypes.data, np.zeros(8).ctypes.data

    def call(img=p, h=8, w=8, pitch=24, cn=3, depth=0, prm=None, ws=p, o=out):
        return L.v1c_fit_circle_async(0, None, img, h, w, pitch, cn, depth, prm, ws, o)

    for kw, word in (({"img": None}, b"NULL"), ({"ws": None}, b"NULL"), ({"o": None}, b"NULL"), ({"cn": 2}, b"cn"), ({"depth": 5}, b"depth"),
                     ({"h": 0}, b"size"), ({"w": 40000}, b"size"), ({"pitch": 23}, b"pitch"), ({"depth": 2, "pitch": 49}, b"even"),
                     ({"depth": 2, "img": p + 1, "pitch": 48}, b"even"), ({"ws": p + 2}, b"aligned"), ({"o": out + 4}, b"aligned")):
        assert call(**kw) == _abi.E_INVALID and word in L.v1c_last_error(), kw
    ok = dict(threshold=10, run=4, rounds=4, min_points=8)
    for bad in (dict(threshold=-1), dict(threshold=65536), dict(run=0), dict(run=65), dict(rounds=-1), dict(rounds=9), dict(min_points=2)):
        prm = Params(**dict(ok, **bad), tol16=(C.c_int32 * 8)(*[24] * 8))
        assert call(prm=C.byref(prm)) == _abi.E_INVALID and b"parameter" in L.v1c_last_error(), bad
    prm = Params(**ok, tol16=(C.c_int32 * 8)(24, 24, 0, 24))
    assert call(prm=C.byref(prm)) == _abi.E_INVALID and b"tol16" in L.v1c_last_error()
    n = C.c_int32()
    pts = np.zeros(3 * 32, np.int32)
    assert L.v1c_fit_circle(0, None, p, 8, 8, 24, 3, 0, None, p, out, pts.ctypes.data, -1, C.byref(n)) == _abi.E_INVALID
    assert L.v1c_fit_circle(0, None, p, 8, 8, 24, 3, 0, None, p, out, pts.ctypes.data, 32, None) == _abi.E_INVALID
    assert L.v1c_fit_circle(0, None, None, 8, 8, 24, 3, 0, None, p, out, None, 0, None) == _abi.E_INVALID


# ---- the Python plumbing of center= and radius="fit", no device --------------------------------------------------------------------------
def _chains():
    import vr180_convert_amd as V

    return {"default": V.EquirectangularEncoder() * V.FisheyeDecoder("equidistant"),
            "zoom": V.ZoomTransformer(1.3) * V.FisheyeDecoder("equidistant")}


def _ops(chain):
    return [(o.opcode, o.iparam, o.nparam, list(o.p)) for o in chain.ops[: chain.n_ops]]


def test_center_none_lowers_to_todays_op_list():
    """field for field: today's Denormalize centre is two ints, (W_in // 2, H_in // 2); center=None must hand the op the same values,
    and an explicit centre changes p[2], p[3] of the Denormalize op and nothing else"""
    from vr180_convert_amd import _abi
    from vr180_convert_amd.chain import DenormalizeTransformer, NormalizeTransformer, lower_for_get_map

    for t in _chains().values():
        for size_in, size_out in (((80, 96), (64, 64)), ((513, 641), (512, 256))):
            today = (NormalizeTransformer() * t * DenormalizeTransformer(scale=(30.5, 30.5), center=(size_in[1] // 2, size_in[0] // 2))
                     ).lower((size_out[1], size_out[0]))
            ch = lower_for_get_map(t, radius=30.5, size_input=size_in, size_output=size_out)
            assert _ops(ch) == [(o.opcode, o.iparam, o.nparam, list(o.p)) for o in today]
            assert bytes(ch) == bytes(lower_for_get_map(t, radius=30.5, size_input=size_in, size_output=size_out, center=None))
            off = lower_for_get_map(t, radius=30.5, size_input=size_in, size_output=size_out, center=(52.25, 37.5))
            a, b = _ops(ch), _ops(off)
            assert a[:-1] == b[:-1] and b[-1][0] == _abi.OP_DENORMALIZE
            assert b[-1][3][:4] == [30.5, 30.5, 52.25, 37.5] and a[-1][3][:2] == b[-1][3][:2] and a[-1][3][4:] == b[-1][3][4:]
    with pytest.raises(ValueError):
        lower_for_get_map(t, radius=30.5, size_input=(80, 96), size_output=(64, 64), center="auto")
    with pytest.raises(ValueError):
        lower_for_get_map(t, radius=30.5, size_input=(80, 96), size_output=(64, 64), center=(float("nan"), 1.0))


def test_cache_keys_without_a_centre_are_todays():
    from vr180_convert_amd import remapper

    t = _chains()["default"]
    remapper.clear_caches()
    remapper._lower_cached(t, radius=30.5, size_input=(80, 96), size_output=(64, 64))
    k0 = list(remapper._LOWERED)
    assert k0 == [(remapper._transformer_key(t), (30.5).hex(), (80, 96), (64, 64))]
    remapper._lower_cached(t, radius=30.5, size_input=(80, 96), size_output=(64, 64), center=(52.25, 37.5))
    remapper._lower_cached(t, radius=30.5, size_input=(80, 96), size_output=(64, 64), center=(52.25, 37.5))
    remapper._lower_cached(t, radius=30.5, size_input=(80, 96), size_output=(64, 64), center=(52.5, 37.5))
    assert len(remapper._LOWERED) == 3 and list(remapper._LOWERED)[0] == k0[0]
    remapper.clear_caches()


def test_explicit_centre_gives_the_numpy_chains_map():
    """_host_map with a centre is the NumPy chain with that DenormalizeTransformer; a centre of (W // 2, H // 2) is today's map"""
    from vr180_convert_amd import remapper
    from vr180_convert_amd.chain import DenormalizeTransformer, NormalizeTransformer

    for t in _chains().values():
        xm, ym = remapper._host_map(t, radius=30.5, size_input=(80, 96), size_output=(64, 48), center=(52.25, 37.5))
        xx, yy = np.meshgrid(np.arange(64), np.arange(48))
        wx, wy = (NormalizeTransformer() * t * DenormalizeTransformer(scale=(30.5, 30.5), center=(52.25, 37.5))).transform(xx, yy)
        assert np.array_equal(xm, wx.astype(np.float32), equal_nan=True) and np.array_equal(ym, wy.astype(np.float32), equal_nan=True)
        a = remapper._host_map(t, radius=30.5, size_input=(80, 96), size_output=(64, 48))
        b = remapper._host_map(t, radius=30.5, size_input=(80, 96), size_output=(64, 48), center=(48, 40))
        assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


class _Shape:
    def __init__(self, *shape):
        self.shape, self.dtype = shape, "u8"


def test_group_units_splits_by_centre_and_shares_where_they_agree():
    from vr180_convert_amd import remapper

    t = _chains()["default"]
    srcs, dsts = [_Shape(80, 96, 3)] * 4, [_Shape(64, 64, 3)] * 4
    g0, hm = remapper.group_units(t, srcs, dsts, radius=30.0)
    assert len(g0) == 1 and not hm
    g1, _ = remapper.group_units(t, srcs, dsts, radius=30.0, center=(52.25, 37.5))
    assert len(g1) == 1 and g1[0].index == [0, 1, 2, 3] and bytes(g1[0].chain) != bytes(g0[0].chain)
    g2, _ = remapper.group_units(t, srcs, dsts, radius=30.0, center=[(52.25, 37.5), None, (52.25, 37.5), (40.0, 41.0)])
    assert [g.index for g in g2] == [[0, 2], [1], [3]]
    assert bytes(g2[0].chain) == bytes(g1[0].chain) and bytes(g2[1].chain) == bytes(g0[0].chain)
    for bad in ([(1.0, 2.0)] * 3, [(1.0, 2.0, 3.0)] * 4, "auto"):
        with pytest.raises(ValueError):
            remapper.group_units(t, srcs, dsts, radius=30.0, center=bad)
    assert remapper.per_unit_centers(None, 3) is None and remapper.per_unit_centers([None, None], 2) is None
    assert remapper.per_unit_centers((1, 2), 2) == [(1.0, 2.0), (1.0, 2.0)]


def test_rounding_of_fitted_centres_and_radii():
    from vr180_convert_amd import circle, remapper

    assert circle.round_center(1341.0082, 1123.9889) == (1341.0, 1124.0)
    assert circle.round_center(10.124, 10.125) == (10.0, 10.25) and circle.round_center(10.374, 10.376) == (10.25, 10.5)
    assert circle.round_radius(1027.6189) == 1027.5 and circle.round_radius(1027.75) == 1028.0 and circle.round_radius(30.2) == 30.0
    fits = [circle.Circle(1341.0082, 1123.9889, 1027.6189, 8192, 7601, 0.46), circle.Circle(1340.9, 1124.2, 1027.8, 8000, 7000, 0.5)]
    imgs = [np.zeros((4, 4, 3), np.uint8)] * 2
    # the frames of one rig: fitted centres a tenth of a pixel apart land on one grid point, hence one plan
    assert remapper.fit_centers("auto", imgs, fits=fits) == [(1341.0, 1124.0), (1341.0, 1124.25)]
    assert remapper.fit_centers("auto", imgs, fits=fits[:1] * 2) == [(1341.0, 1124.0)] * 2
    assert remapper.get_radius_smart("fit", imgs, fits=fits) == 1028.0  # the maximum, on get_radius's grid of 1/2 px, positive
    with pytest.raises(ValueError):
        remapper.fit_centers("middle", imgs, fits=fits)


def test_auto_centre_is_refused_under_capture_and_with_the_device_resident_radius(monkeypatch):
    import torch

    from vr180_convert_amd import circle, remapper

    t = _chains()["default"]
    img = torch.zeros((8, 8, 3), dtype=torch.uint8)
    called = []
    monkeypatch.setattr(circle, "fit_circle", lambda im, **k: called.append(1) or circle.Circle(4.0, 4.0, 3.0, 16, 16, 0.1))
    with pytest.raises(NotImplementedError, match="auto_radius_on_device"):
        remapper.apply_lr_tensors(t, img, img, size_output=(8, 8), radius="auto", auto_radius_on_device=True, center="auto",
                                  out=torch.zeros((8, 16, 3), dtype=torch.uint8))
    monkeypatch.setattr(remapper, "_capturing", lambda: True)
    with pytest.raises(NotImplementedError, match="captured"):
        remapper.apply_lr_tensors(t, img, img, size_output=(8, 8), radius=3.0, center="auto", out=torch.zeros((8, 16, 3), dtype=torch.uint8))
    with pytest.raises(NotImplementedError, match="captured"):
        remapper.remap_tensors(t, [img], [img], radius=3.0, center="auto")
    with pytest.raises(NotImplementedError, match="captured"):
        remapper.fit_centers("auto", [img])
    assert not called  # refused before anything is fitted
    with pytest.raises(NotImplementedError):
        remapper.remap_tensors_auto(t, [img], [img], center="auto")
    with pytest.raises(NotImplementedError):
        remapper.remap_tensors_auto(t, [img], [img], center=[(1.0, 2.0)])


def test_explicit_centres_reach_the_launches(monkeypatch):
    """apply_lr_tensors hands an explicit centre, a pair of them and fitted ones on to remap_tensors; radius='auto' keeps its value"""
    import torch

    from vr180_convert_amd import circle, remapper

    t = _chains()["default"]
    img = torch.zeros((8, 8, 3), dtype=torch.uint8)
    out = torch.zeros((8, 16, 3), dtype=torch.uint8)
    seen = []
    monkeypatch.setattr(remapper, "remap_tensors", lambda tr, s, d, **k: seen.append((k["radius"], k.get("center"), k.get("size_input"))))
    monkeypatch.setattr(remapper, "_get_radius_any", lambda im, threshold=10: -3.5)
    monkeypatch.setattr(remapper, "_capturing", lambda: False)
    fits = iter([circle.Circle(4.1, 3.9, 3.2, 16, 16, 0.1), circle.Circle(5.6, 4.4, 3.3, 16, 16, 0.1)] * 2)
    monkeypatch.setattr(circle, "fit_circle", lambda im, **k: next(fits))
    remapper.apply_lr_tensors(t, img, img, out=out, size_output=(8, 8), radius=3.0, center=(5.0, 4.5))
    remapper.apply_lr_tensors(t, img, img, out=out, size_output=(8, 8), radius="auto", auto_radius_on_device=False,
                              center=((5.0, 4.5), (3.0, 4.0)))
    remapper.apply_lr_tensors(t, img, img, out=out, size_output=(8, 8), radius="auto", auto_radius_on_device=False, center="auto")
    remapper.apply_lr_tensors(t, img, img, out=out, size_output=(8, 8), radius="fit", center="auto")
    assert seen == [(3.0, [(5.0, 4.5), (5.0, 4.5)], (8, 8)), (-3.5, [(5.0, 4.5), (3.0, 4.0)], (8, 8)),
                    (-3.5, [(4.0, 4.0), (5.5, 4.5)], (8, 8)), (3.5, [(4.0, 4.0), (5.5, 4.5)], (8, 8))]


def test_match_lr_sends_the_points_back_through_the_given_centres(monkeypatch):
    from vr180_convert_amd import calibration, circle
    from vr180_convert_amd.chain import DenormalizeTransformer, FisheyeDecoder, equidistant_to_3d

    dec = FisheyeDecoder("equidistant")
    imgs = [np.zeros((80, 96, 3), np.uint8)] * 2
    pl, pr = [(30, 40), (50, 20), (60, 61)], [(33, 41), (52, 22), (58, 60)]

    def rays(pts, c):
        p = np.array(pts)
        x, y = (dec * DenormalizeTransformer(scale=(30.0, 30.0), center=c)).inverse_transform(p[:, 0].astype(np.float32), p[:, 1].astype(np.float32))
        return equidistant_to_3d(x, y)

    a = calibration.match_lr(dec, pl, pr, imgs, radius=30.0)
    assert np.array_equal(a[0], rays(pl, (48, 40))) and np.array_equal(a[1], rays(pr, (48, 40)))
    b = calibration.match_lr(dec, pl, pr, imgs, radius=30.0, center=(52.25, 37.5))
    assert np.array_equal(b[0], rays(pl, (52.25, 37.5))) and np.array_equal(b[1], rays(pr, (52.25, 37.5)))
    c = calibration.match_lr(dec, pl, pr, imgs, radius=30.0, center=((52.25, 37.5), (44.0, 41.75)))
    assert np.array_equal(c[0], rays(pl, (52.25, 37.5))) and np.array_equal(c[1], rays(pr, (44.0, 41.75)))
    d = calibration.match_lr((dec, dec), pl, pr, imgs, radius=30.0, center=((52.25, 37.5), (44.0, 41.75)))
    assert np.array_equal(d[0], c[0]) and np.array_equal(d[1], c[1])
    fits = iter([circle.Circle(52.3, 37.4, 30.2, 99, 99, 0.1), circle.Circle(44.1, 41.8, 29.9, 99, 99, 0.1)])
    monkeypatch.setattr(circle, "fit_circle", lambda im, **k: next(fits))
    e = calibration.match_lr(dec, pl, pr, imgs, radius=30.0, center="auto")
    assert np.array_equal(e[0], c[0]) and np.array_equal(e[1], c[1])


def test_cli_parses_center_and_radius_fit(tmp_path, monkeypatch):
    import typer
    from typer.testing import CliRunner

    from vr180_convert_amd import _io, cli, remapper, synth

    assert cli.parse_center("") is None and cli.parse_center("auto") == "auto" and cli.parse_center("10.5,20") == (10.5, 20.0)
    assert cli.parse_center("1,2;3,4.25") == ((1.0, 2.0), (3.0, 4.25)) and cli.parse_center("1,2;3,4.25", swap=True) == ((3.0, 4.25), (1.0, 2.0))
    assert cli.parse_center("1,2", swap=True) == (1.0, 2.0)
    for bad in ("1", "1,2,3", "1,2;3,4;5,6", "a,b", "centre"):
        with pytest.raises(typer.BadParameter):
            cli.parse_center(bad)
    with pytest.raises(typer.BadParameter):
        cli.parse_center("1,2;3,4", pair=False)
    assert cli.parse_radius("fit") == "fit" and cli.parse_radius("auto") == "auto" and cli.parse_radius("12.5") == 12.5
    seen = []
    monkeypatch.setattr(remapper, "apply_lr", lambda *a, **k: seen.append(("lr", k["radius"], k.get("center", "absent"))))
    monkeypatch.setattr(remapper, "apply", lambda *a, **k: seen.append(("s", k["radius"], k.get("center", "absent"))))
    img = tmp_path / "a.png"
    _io.imwrite(img, synth.pattern(64, 64))
    run = CliRunner().invoke
    out = ["--size", "32x32", "--out-path", str(tmp_path / "o.png")]
    assert run(cli.app, ["lr", str(img), str(img), "--radius", "max", *out]).exit_code == 0
    assert run(cli.app, ["lr", str(img), str(img), "--radius", "fit", "--center", "auto", *out]).exit_code == 0
    assert run(cli.app, ["lr", str(img), str(img), "--radius", "30", "--center", "1,2;3,4", *out]).exit_code == 0
    assert run(cli.app, ["lr", str(img), str(img), "--radius", "30", "--center", "1,2;3,4", "--swap", *out]).exit_code == 0
    assert run(cli.app, ["s", str(img), "--radius", "fit", "--center", "7.5,8", *out]).exit_code == 0
    assert run(cli.app, ["s", str(img), "--radius", "max", *out]).exit_code == 0
    assert run(cli.app, ["s", str(img), "--center", "1,2;3,4", *out]).exit_code != 0
    assert run(cli.app, ["lr", str(img), str(img), "--center", "nowhere", *out]).exit_code != 0
    assert seen == [("lr", "max", "absent"), ("lr", "fit", "auto"), ("lr", 30.0, ((1.0, 2.0), (3.0, 4.0))), ("lr", 30.0, ((3.0, 4.0), (1.0, 2.0))),
                    ("s", "fit", (7.5, 8.0)), ("s", "max", "absent")]
