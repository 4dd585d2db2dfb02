"""The vignetting correction without a device: the restatement (tests/vignette_ref.py) against a host build
of vignette_core.hpp driven through the kernels' decomposition (tests/host_vignette/vignette_emul.hip), the same program under the
address and undefined-behaviour sanitizers, the derived distance of the integer rule from float64, what the tables promise (clamps,
the identity), the round trip flat field -> fit -> tables -> apply, the argument checks of the C ABI and of the Python entries, and
the strings of the CLI."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import vignette_cases as VC
import vignette_ref as R

ROOT = Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "host_vignette" / "vignette_emul.hip"
NAMES = sorted(VC.shared_cases())


@pytest.fixture(scope="module")
def vig_emul(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_vignette") / "libvignette_emul.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-fno-fast-math", "-o", str(out),
                    str(HARNESS)], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(out))
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    lib.vignette_emul_apply.argtypes = [vp, i64, vp, i64, i32, i32, i32, i32, vp, vp, i32]
    lib.vignette_emul_apply.restype = None
    lib.vignette_emul_rings.argtypes = [vp, i64, i32, i32, i32, i32, vp, i32, vp]
    lib.vignette_emul_rings.restype = None
    lib.vignette_emul_max_r2.argtypes = [i32, i32, i32, i32]
    lib.vignette_emul_max_r2.restype = i64
    return lib


def _emul(lib, case, blocks=3):
    """the case on a copy of its base: (result, ring record, the base afterwards)"""
    base = case.base.copy()
    h, w, cn = case.shape
    es = np.dtype(case.dtype).itemsize
    img = case.view(base)
    cx, cy, scale, shift, R2 = VC.geometry(case)
    tab = np.ascontiguousarray(VC.tables(case))
    rec = np.full((case.rings, 4), -1, np.int64)
    prm = np.array([cx, cy, R2, case.rings, case.lo, case.hi], np.int64)
    lib.vignette_emul_rings(img.ctypes.data, case.pitch, h, w, cn, es, prm.ctypes.data, blocks, rec.ctypes.data)
    out = img if case.inplace else np.full((h, w, cn), VC.FILL * 0x0101 & (0xFF if es == 1 else 0xFFFF), case.dtype)
    geom = np.array([cx, cy, scale, shift], np.int64)
    lib.vignette_emul_apply(img.ctypes.data, case.pitch, out.ctypes.data, out.strides[0], h, w, cn, es, geom.ctypes.data, tab.ctypes.data, blocks)
    return np.array(out), rec, base


def same(got, want, case):
    result, rec, base = got
    wresult, wrec = want
    assert np.array_equal(rec, wrec)
    assert np.array_equal(result, wresult)
    assert np.array_equal(base, VC.expected_base(case, wresult))  # every byte around the image and between its rows is as it was


@pytest.mark.parametrize("name", NAMES)
def test_product_host_code_equals_restatement(vig_emul, name):
    case = VC.shared_cases()[name]
    same(_emul(vig_emul, case), VC.reference(name), case)


def test_the_decomposition_does_not_show(vig_emul):
    """one workgroup or seven: the sums are integers"""
    for name in ("sbs_odd_uint8", "rings_1024_uint16"):
        case = VC.shared_cases()[name]
        for blocks in (1, 7):
            same(_emul(vig_emul, case, blocks=blocks), VC.reference(name), case)


def test_saturated_wide_frame_passes_the_flushes(vig_emul):
    """the 1200 x 1200 uint16 frame of all 65535 through ONE workgroup: 357 rounds, so every thread's items pass eleven flushes, and a
    ring's sum passes 2^32 -- the overflow case of the 32-bit copies"""
    img = np.full((1200, 1200, 3), 65535, np.uint16)
    case = VC.carve(img, radius=900.0, rings=16, hi=65535)
    want = VC.reference_of(case)
    assert want[1][:, :3].max() > 1 << 32 and want[1][:, 3].sum() == 1200 * 1200
    same(_emul(vig_emul, case, blocks=1), want, case)


def test_the_cases_cover_what_they_are_meant_to():
    refs = {n: VC.reference(n) for n in NAMES}
    cases = VC.shared_cases()
    for n in ("identity_uint8", "identity_uint16"):
        assert np.array_equal(refs[n][0], cases[n].view()) and (VC.tables(cases[n]) == 1 << 14).all()
    for n in ("masked_out_uint8", "masked_out_uint16"):
        assert not refs[n][1].any()
    for n in ("saturates_uint8", "saturates_uint16"):
        top = 255 if n.endswith("8") else 65535
        assert (refs[n][0] == top).mean() > 0.2 and (refs[n][0] < top).any()
    for n in ("radius_2_uint8", "radius_2_uint16"):
        cx, cy, scale, shift, R2 = VC.geometry(cases[n])
        idx, f = R.position(R.r2_of(37, 83, cx, cy), scale, shift)
        assert R2 == 4 and (idx == 1023).mean() > 0.9 and set(f[idx == 1023]) == {255} and len(np.unique(idx)) >= 3
        assert refs[n][1][:, 3].sum() == int((R.r2_of(37, 83, cx, cy) < 4).sum()) > 4
    case = cases["cn4_uint16"]
    assert np.array_equal(refs["cn4_uint16"][0][..., 3], case.view()[..., 3]) and not np.array_equal(refs["cn4_uint16"][0], case.view())
    assert not refs["cn1_uint8"][1][:, [0, 2]].any() and refs["cn1_uint8"][1][:, 1].any()
    for n in NAMES:
        if "center_" in n:
            h, w, _ = cases[n].shape
            assert not (0 <= cases[n].center[0] < w and 0 <= cases[n].center[1] < h)


# ---- the fixed point cannot overflow ----------------------------------------------------------------------------------------------------
def test_widths_hold_for_every_frame_the_entries_accept(vig_emul):
    """r2 < 2^34 for every frame up to 32767 x 32767 with the centre up to one frame size outside it, scale < 2^30: the product stays in
    64 unsigned bits; and the strip of the GPU suite computes what Python's integers give"""
    from vr180_convert_amd import vignette as V

    worst = 0
    for w, h in ((32767, 32767), (32767, 1), (1, 32767)):
        for cx in (-w, 2 * w - 1, w // 2):
            for cy in (-h, 2 * h - 1):
                worst = max(worst, int(vig_emul.vignette_emul_max_r2(h, w, cx, cy)))
                assert int(vig_emul.vignette_emul_max_r2(h, w, cx, cy)) == max((x - cx) ** 2 + (y - cy) ** 2 for x in (0, w - 1) for y in (0, h - 1))
    assert worst == 2 * 65533 ** 2 < 1 << V.R2_BITS
    for radius in (1.0, 2.0, 3.7, 100.0, 2048.0, 46340.0, 92681.0):
        scale, shift = V.table_scale(radius)
        assert 1 << 29 <= scale < 1 << 30 and 0 <= shift <= 62
        assert worst * scale < 1 << 64
        exact = 256 * 1024 / radius ** 2
        assert abs(scale / 2.0 ** shift / exact - 1) <= 2.0 ** -29
    for bad in (0.0, float("nan"), float("inf"), 1e-9, 1e12):
        with pytest.raises(ValueError):
            V.table_scale(bad)
    # the strip: Python ints against the restatement's uint64
    cx, cy, scale, shift = 32766, 1, *V.table_scale(33000.0)
    r2 = R.r2_of(2, 32767, cx, cy)
    idx, f = R.position(r2, scale, shift)
    for x in (0, 1, 12345, 32766):
        q = (int(r2[0, x]) * scale) >> shift
        assert (idx[0, x], f[0, x]) == ((q >> 8, q & 255) if q >> 8 < 1024 else (1023, 255))
    assert int(r2.max()) * scale > 1 << 59  # (past 32 bits, and past the 53 of a double)


# ---- the distance from float64, derived from the formats ---------------------------------------------------
def _derived_bound(v, maxv, bins=1024):
    """0.5 for the final rounding, and maxv times the gain's own error: 2^-15 for an entry's rounding to Q14, 2^-15 for the rounding
    of the interpolated gain, D^2 / 8 max|g''| for the linear interpolation over an interval D = 1 / bins of rho^2, and
    D max|g'| (1 / 256 + 2^-12) for the position: the fraction is cut to 1/256 of an interval, and the multiplier's rounding (2^-29
    of q < 2^18 + 2^8) moves it by less than 2^-11 of 1/256... taken as 2^-12 of an interval.  g', g'' from the polynomial's own
    derivatives in float64, over [0, 1]."""
    t = np.linspace(0.0, 1.0, 200001)
    worst = 0.0
    for k1, k2, k3 in (v.blue, v.green, v.red):
        V = 1 + t * (k1 + t * (k2 + t * k3))
        V1 = k1 + t * (2 * k2 + 3 * k3 * t)
        V2 = 2 * k2 + 6 * k3 * t
        p = -1.0 / v.gamma
        g1 = p * V ** (p - 1) * V1
        g2 = p * (p - 1) * V ** (p - 2) * V1 ** 2 + p * V ** (p - 1) * V2
        D = 1.0 / bins
        worst = max(worst, 2.0 ** -15 + 2.0 ** -15 + D * D / 8 * np.abs(g2).max() + D * np.abs(g1).max() * (1 / 256 + 2.0 ** -12))
    return 0.5 + maxv * worst


@pytest.mark.parametrize("coefs", [VC.STRONG, VC.ENCODED, (((0.2, -0.1, 0.0),) * 3, 1.0)], ids=["strong", "gamma22", "brightening"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_the_integer_rule_is_within_its_derived_distance_of_float64(coefs, dtype):
    from vr180_convert_amd import vignette as V

    case = VC.carve(VC.noise(61, 97, 3, dtype, 5, lo=0, hi=255 if dtype == np.uint8 else 65535), radius=52.3, center=(47, 29), coefs=coefs)
    v = case.vignette()
    maxv = 255 if dtype == np.uint8 else 65535
    cx, cy, scale, shift, _ = VC.geometry(case)
    got = R.apply(case.view(), V.gain_tables(v), cx, cy, scale, shift).astype(np.float64)
    rho2 = R.r2_of(61, 97, cx, cy) / 52.3 ** 2
    g = v.gain(rho2)
    assert g.max() < V.GAIN_MAX and (rho2 > 1).any()
    exact = np.minimum(maxv, case.view().astype(np.float64) * np.moveaxis(g, 0, 2))
    bound = _derived_bound(v, maxv)
    err = np.abs(got - exact).max()
    print(f"{np.dtype(dtype).name}: largest distance {err:.4f}, derived bound {bound:.4f}")
    assert bound < (0.6 if dtype == np.uint8 else 12.0)  # (the bound itself says something: about half a level, and a few of 65535)
    assert err <= bound


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------
def test_tables_clamp_hold_and_keep_the_identity():
    from vr180_convert_amd import vignette as V

    assert (V.gain_tables(V.Vignette()) == 1 << 14).all() and V.gain_tables(V.Vignette()).shape == (3, 1025)
    assert V.gain_tables(V.Vignette(), bins=16).shape == (3, 17)
    # a falloff to zero and below: the gain stops at 65535 / 2^14, just under two stops, wherever V turns over
    t = V.gain_tables(V.Vignette((-1.2, 0.0, 0.0)))
    assert t.dtype == np.uint16 and t.max() == 65535 and t[0, 0] == 1 << 14 and (np.diff(t.astype(int), axis=1) >= 0).all()
    # a brightening model is not clamped at one: gains below 1 are what it asks for
    assert V.gain_tables(V.Vignette((0.5, 0.0, 0.0)))[1, -1] == round(16384 / 1.5)
    # beyond rho = 1 the rim's value is held, whatever the polynomial does there
    v = V.Vignette((-0.3, 0.0, -4.0))
    wide = V.gain_tables(v, rho2_max=2.0)
    assert (wide[:, 512:] == wide[:, 512:513]).all() and wide[1, 512] == V.gain_tables(v)[1, 1024]
    # per channel, BGR
    t = V.gain_tables(V.Vignette((-0.1, 0, 0), red=(-0.3, 0, 0), blue=(-0.2, 0, 0)))
    assert t[0, -1] == round(16384 / 0.8) and t[1, -1] == round(16384 / 0.9) and t[2, -1] == round(16384 / 0.7)
    # gamma folds the encoding into the table
    assert V.gain_tables(V.Vignette((-0.5, 0, 0), gamma=2.0))[1, -1] == round(16384 * 2 ** 0.5)
    # a measured curve taken as it is
    m = V.Vignette.from_rings([0.0, 0.5, 1.0], [1.0, 1.5, 3.0])
    tm = V.gain_tables(m)
    assert tm[0, 0] == 16384 and tm[2, 512] == 24576 and tm[1, 1024] == 49152 and tm[1, 256] == 20480


def test_identity_leaves_every_pixel_as_it_is():
    from vr180_convert_amd import vignette as V

    for dtype in (np.uint8, np.uint16):
        img = VC.noise(23, 41, 4, dtype, 3, lo=0, hi=255 if dtype == np.uint8 else 65535)
        assert np.array_equal(R.apply(img, V.gain_tables(V.Vignette()), 20, 11, *V.table_scale(20.0)), img)


# ---- the round trip ------------------------------------------------------------------------------------------------------------------------
# largest relative deviation of a ring's mean from the flat level after flat field -> fit -> tables -> apply, over rho <= 0.98, measured
# with the restatement over seeds 0..19
RIPPLE = {"uint8": 0.001454, "uint16": 0.001450}


def _round_trip(dtype, seed):
    from vr180_convert_amd import vignette as V

    h = w = 257
    center, radius = (128, 127), 126.0
    top = 255 if dtype == np.uint8 else 65535
    level = 0.8 * top
    truth = VC.carve(np.zeros((1, 1, 3), dtype), coefs=VC.STRONG).vignette()
    flat = VC.flat_field(truth, h, w, center, radius, level, dtype, seed, sigma=0.004 * top)
    R2 = V.ring_r2(radius)
    lo, hi = V.default_mask(dtype)
    fit = V.fit_rings(R.rings(flat, *center, R2, 256, lo, hi))
    g = V.geometry(h, w, center, radius)
    out = R.apply(flat, V.gain_tables(fit), g.cx, g.cy, g.scale, g.shift)
    rec = R.rings(out, *center, int(R2 * 0.98 ** 2), 64, 1, top)
    means = rec[:, :3] / rec[:, 3:4]
    return float(np.abs(means / level - 1).max()), fit


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_round_trip_is_flat_again(dtype):
    name = np.dtype(dtype).name
    seen = []
    for seed in range(20):
        ripple, fit = _round_trip(dtype, seed)
        seen.append(ripple)
        for got, want in zip((fit.blue, fit.green, fit.red), VC.STRONG[0]):
            assert abs(sum(got) - sum(want)) < 0.02  # (V at the rim: the coefficients trade against each other, their sum does not)
    print(f"{name}: ripple over 20 seeds {min(seen):.5f} .. {max(seen):.5f}")
    assert max(seen) <= 2 * RIPPLE[name]


def test_a_masked_out_frame_gives_a_clear_error():
    from vr180_convert_amd import vignette as V

    rec = R.rings(np.zeros((37, 83, 3), np.uint8), 41, 18, 44 * 44, 64, 10, 254)
    assert not rec.any()
    with np.errstate(all="raise"):  # nothing is divided by zero on the way
        with pytest.raises(ValueError, match="rings hold"):
            V.fit_rings(rec)


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------
def test_model_validation():
    from vr180_convert_amd import vignette as V

    for bad in (dict(coefs=(1, 2)), dict(coefs=(1, 2, 3, 4)), dict(coefs=(0, float("nan"), 0)), dict(red=(0, float("inf"), 0)),
                dict(gamma=0), dict(gamma=-1.0), dict(gamma=float("nan")), dict(coefs="abc"), dict(green=[1])):
        with pytest.raises(ValueError):
            V.Vignette(**bad)
    with pytest.raises(ValueError):
        V.Vignette.from_rings([0, 0.5], [1.0, 1.1, 1.2])
    with pytest.raises(TypeError):
        V.as_per_unit([V.Vignette()] * 3, 2)
    with pytest.raises(TypeError):
        V.as_per_unit("-0.3,0,0", 1)


def test_float32_is_refused_before_any_launch():
    import torch

    from vr180_convert_amd import vignette as V

    class Fake(torch.Tensor):  # a CPU tensor that says it is on the device: the dtype check comes before anything is launched
        is_cuda = True

    t = torch.zeros((4, 4, 3), dtype=torch.float32).as_subclass(Fake)
    with pytest.raises(TypeError, match="uint8 and uint16"):
        V.apply_vignette_tensor(t, V.Vignette(), radius=2.0)
    with pytest.raises(TypeError, match="uint8 and uint16"):
        V.vignette_rings_tensor(t, radius=2.0)
    with pytest.raises(TypeError, match="uint8 and uint16"):
        V.fit_vignette(t, radius=2.0)
    with pytest.raises(TypeError, match="uint8 and uint16"):
        V.fit_vignette(np.zeros((4, 4, 3), np.float32), radius=2.0)


class Geom(C.Structure):
    _fields_ = [("cx", C.c_int32), ("cy", C.c_int32), ("scale", C.c_uint32), ("shift", C.c_int32)]


class RingParams(C.Structure):
    _fields_ = [("cx", C.c_int32), ("cy", C.c_int32), ("r2", C.c_int64), ("rings", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32),
                ("reserved", C.c_int32)]


def test_argument_errors_come_before_any_device_call(product_lib):
    from vr180_convert_amd import _abi
    from vr180_convert_amd import vignette as V

    assert C.sizeof(V.VignetteGeom) == C.sizeof(Geom) == 16 and C.sizeof(V.VignetteRingParams) == C.sizeof(RingParams) == 32
    L = product_lib
    buf = np.zeros(16384, np.uint8)
    p = buf.ctypes.data - buf.ctypes.data % 16 + 16
    good = dict(cx=4, cy=4, scale=1 << 29, shift=20)

    def apply(src=p, sp=24, dst=p + 1024, dp=24, h=8, w=8, cn=3, es=1, geom=good, tab=p + 2048):
        return L.v1c_vignette_apply_async(0, None, src, sp, dst, dp, h, w, cn, es, None if geom is None else C.byref(Geom(**geom)), tab)

    for kw, word in (({"src": None}, b"NULL"), ({"dst": None}, b"NULL"), ({"geom": None}, b"NULL"), ({"tab": None}, b"NULL"),
                     ({"cn": 2}, b"cn"), ({"es": 4}, b"elem_bytes"), ({"es": 0}, b"elem_bytes"), ({"h": 0}, b"size"), ({"w": 32768}, b"size"),
                     ({"sp": 23}, b"pitch"), ({"dp": 0}, b"pitch"), ({"es": 2, "sp": 49, "dp": 48}, b"aligned"),
                     ({"es": 2, "sp": 48, "dp": 48, "src": p + 1}, b"aligned"), ({"tab": p + 2049}, b"aligned"),
                     ({"geom": dict(good, cx=16)}, b"centre"), ({"geom": dict(good, cy=-9)}, b"centre"),
                     ({"geom": dict(good, scale=0)}, b"geometry"), ({"geom": dict(good, scale=1 << 30)}, b"geometry"),
                     ({"geom": dict(good, shift=63)}, b"geometry"), ({"geom": dict(good, shift=-1)}, b"geometry")):
        assert apply(**kw) == _abi.E_INVALID and word in L.v1c_last_error(), kw
    ok = dict(cx=4, cy=4, r2=16, rings=16, lo=10, hi=254, reserved=0)

    def rings(src=p, sp=24, h=8, w=8, cn=3, es=1, prm=ok, out=p + 4096):
        return L.v1c_vignette_rings_async(0, None, src, sp, h, w, cn, es, None if prm is None else C.byref(RingParams(**prm)), out)

    for kw, word in (({"src": None}, b"NULL"), ({"prm": None}, b"NULL"), ({"out": None}, b"NULL"), ({"cn": 5}, b"cn"), ({"sp": 8}, b"pitch"),
                     ({"out": p + 4100}, b"aligned"), ({"prm": dict(ok, cx=-9)}, b"centre")):
        assert rings(**kw) == _abi.E_INVALID and word in L.v1c_last_error(), kw
    for bad in (dict(rings=15), dict(rings=1025), dict(r2=0), dict(r2=1 << 35), dict(lo=-1), dict(hi=256), dict(lo=200, hi=100)):
        assert rings(prm=dict(ok, **bad)) == _abi.E_INVALID and b"parameter" in L.v1c_last_error(), bad
    assert rings(es=2, sp=48, prm=dict(ok, hi=65536)) == _abi.E_INVALID and rings(es=2, sp=48, prm=dict(ok, hi=65535, cx=-9)) == _abi.E_INVALID


# ---- the Python plumbing of vignette=, no device ------------------------------------------------------------------------------------------
def _chain():
    import vr180_convert_amd as V

    return V.EquirectangularEncoder() * V.FisheyeDecoder("equidistant")


def test_entry_points_refuse_what_they_do_not_serve(monkeypatch):
    import torch

    from vr180_convert_amd import remapper
    from vr180_convert_amd import vignette as V

    called = []
    monkeypatch.setattr(remapper, "_to_device", lambda im, dev: called.append("upload") or im)
    monkeypatch.setattr(remapper, "_device", lambda d=None: torch.device("cpu"))
    v = V.Vignette((-0.3, 0, 0))
    u8 = torch.zeros((8, 8, 3), dtype=torch.uint8)
    f32 = torch.zeros((8, 8, 3), dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="auto_radius_on_device"):
        remapper.apply_lr_tensors(_chain(), u8, u8, size_output=(8, 8), radius="auto", auto_radius_on_device=True, vignette=v)
    with pytest.raises(TypeError, match="uint8 and uint16"):
        remapper.apply_lr_tensors(_chain(), f32, f32, size_output=(8, 8), radius=3.0, vignette=v)
    with pytest.raises(TypeError, match="uint8 and uint16"):
        remapper.remap_tensors(_chain(), [f32], [f32.clone()], radius=3.0, vignette=v)
    with pytest.raises(TypeError, match="one per image"):
        remapper.apply_lr_tensors(_chain(), u8, u8, size_output=(8, 8), radius=3.0, vignette=(v, v, v))
    with pytest.raises(TypeError, match="one Vignette"):  # one map serves every image of apply: one correction
        remapper.apply(_chain(), in_paths=[np.zeros((8, 8, 3), np.uint8)] * 2, size_output=(8, 8), radius=3.0, vignette=[v, v])
    with pytest.raises(TypeError, match="uint8 and uint16"):
        remapper.apply(_chain(), in_paths=[np.zeros((8, 8, 3), np.float32)], size_output=(8, 8), radius=3.0, vignette=v)
    with pytest.raises(TypeError, match="uint8 and uint16"):
        remapper.apply_lr(_chain(), left_path=np.zeros((8, 8, 3), np.float32), right_path=np.zeros((8, 8, 3), np.float32), out_path=None,
                          size_output=(8, 8), radius=3.0, vignette=v)
    assert not called


def test_without_vignette_none_of_it_is_imported(tmp_path):
    code = ("import sys, numpy as np, torch\n"
            "import vr180_convert_amd as V\n"
            "from vr180_convert_amd import remapper, _io\n"
            "remapper._device = lambda d=None: torch.device('cpu')\n"
            "remapper._to_device = lambda im, dev: torch.from_numpy(np.ascontiguousarray(im))\n"
            "remapper.remap_tensors = lambda *a, **k: None\n"
            "_io.imwrite = lambda p, a: None\n"
            "img = np.zeros((8, 8, 3), np.uint8)\n"
            "t = V.EquirectangularEncoder() * V.FisheyeDecoder('equidistant')\n"
            "remapper.apply_lr(t, left_path=img, right_path=img, out_path='o.png', size_output=(8, 8), radius=3.0)\n"
            "assert 'vr180_convert_amd.vignette' not in sys.modules\n"
            "remapper.apply_lr(t, left_path=img, right_path=img, out_path='o.png', size_output=(8, 8), radius=3.0, vignette=None)\n"
            "remapper.apply(t, in_paths=[img], size_output=(8, 8), radius=3.0, vignette=None)\n"
            "from vr180_convert_amd import cli\n"
            "assert 'vr180_convert_amd.vignette' not in sys.modules\n"
            "assert V.Vignette.__module__ == 'vr180_convert_amd.vignette' and 'fit_vignette' in V.__all__ and 'apply_vignette_tensor' in V.__all__\n"
            "assert V.gain_tables is sys.modules['vr180_convert_amd.vignette'].gain_tables\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the CLI's strings -------------------------------------------------------------------------------------------------------------------
def test_cli_strings_parse_and_print_round_trip():
    from vr180_convert_amd import vignette as V

    v = V.parse("-0.3,0.05,-0.01")
    assert v.blue == v.green == v.red == (-0.3, 0.05, -0.01) and v.gamma == 1.0
    v = V.parse("b:-0.3,0,0; r:-0.1,0.2,0", gamma=2.2)
    assert v.blue == (-0.3, 0.0, 0.0) and v.red == (-0.1, 0.2, 0.0) and v.green == (0.0, 0.0, 0.0) and v.gamma == 2.2
    left, right = V.parse_pair("-0.3,0,0|g:-0.2,0,0")
    assert left.red == (-0.3, 0.0, 0.0) and right.green == (-0.2, 0.0, 0.0) and right.red == (0.0, 0.0, 0.0)
    for text in ("", "1,2", "x:1,2,3", "b:1,2,3;b:1,2,3", "1,2,three", "a|b|c", "r:1,2"):
        with pytest.raises(ValueError):
            V.parse_pair(text)
    for v in (V.Vignette((-0.31234567890123, 0.05, 1e-17)), V.Vignette((0, 0, 0), red=(-0.25, 0.125, 1 / 3), blue=(-0.5, 0, 0))):
        back = V.parse(v.spec())
        assert (back.blue, back.green, back.red) == (v.blue, v.green, v.red)  # to the bit


def test_cli_options_reach_the_entries(tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from vr180_convert_amd import _io, cli, remapper, synth
    from vr180_convert_amd import vignette as V

    seen = []
    monkeypatch.setattr(remapper, "apply_lr", lambda *a, **k: seen.append(k.get("vignette", "absent")))
    img = tmp_path / "a.png"
    _io.imwrite(img, synth.pattern(64, 64))
    run = CliRunner().invoke
    out = ["--size", "32x32", "--out-path", str(tmp_path / "o.png"), "--radius", "max"]
    assert run(cli.app, ["lr", str(img), str(img), *out]).exit_code == 0
    assert run(cli.app, ["lr", str(img), str(img), "--vignette", "-0.3,0,0", *out]).exit_code == 0
    assert run(cli.app, ["lr", str(img), str(img), "--vignette", "-0.3,0,0|r:-0.2,0,0", "--vignette-gamma", "2.2", *out]).exit_code == 0
    assert run(cli.app, ["lr", str(img), str(img), "--vignette", "-0.3,0", *out]).exit_code != 0
    assert run(cli.app, ["lr", str(img), str(img), "--vignette", "-0.3,0,0", "--vignette-gamma", "0", *out]).exit_code != 0
    assert seen[0] == "absent" and isinstance(seen[1], V.Vignette) and seen[1].green == (-0.3, 0.0, 0.0)
    assert isinstance(seen[2], tuple) and seen[2][1].red == (-0.2, 0.0, 0.0) and seen[2][0].gamma == 2.2 and len(seen) == 3
    # the fit command prints what --vignette reads
    monkeypatch.setattr(V, "fit_vignette", lambda image, **k: seen.append(k) or V.Vignette((-0.25, 0.5, 0.125), red=(-0.5, 0, 0)))
    r = run(cli.app, ["vignette", str(img), "--center", "auto", "--radius", "fit"])
    assert r.exit_code == 0, r.output
    back = V.parse(r.output.strip().splitlines()[-1])
    assert back.red == (-0.5, 0.0, 0.0) and back.green == (-0.25, 0.5, 0.125)
    assert seen[-1]["center"] == "auto" and seen[-1]["radius"] == "fit"


# ---- the same program under the sanitizers ---------------------------------------------------------------------------------------------------
def test_sanitized_program_over_the_cases(tmp_path):
    """the harness as a program of its own under the address and undefined-behaviour sanitizers: every case from a heap copy of the
    exact size of its base buffer; any report fails the run, and what it prints is the restatement's"""
    exe = tmp_path / "vignette_san"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fno-fast-math", "-DVIGNETTE_MAIN", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(HARNESS)], check=True,
                   capture_output=True, timeout=600)
    lines = []
    for k, name in enumerate(NAMES):
        case = VC.shared_cases()[name]
        p, tp = tmp_path / f"case_{k}.raw", tmp_path / f"case_{k}.tab"
        p.write_bytes(case.base.tobytes())
        tp.write_bytes(np.ascontiguousarray(VC.tables(case)).tobytes())
        h, w, cn = case.shape
        cx, cy, scale, shift, R2 = VC.geometry(case)
        lines.append(" ".join(str(v) for v in [h, w, cn, np.dtype(case.dtype).itemsize, case.off, case.pitch, int(case.inplace), cx, cy, scale,
                                               shift, R2, case.rings, case.lo, case.hi, 2, p, tp]))
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(tmp_path / "list.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    rows = r.stdout.strip().split("\n")
    assert len(rows) == len(NAMES)
    for name, row in zip(NAMES, rows):
        f = row.split()
        want = VC.reference(name)
        nrec = want[1].size
        assert np.array_equal(np.array(f[:nrec], np.int64).reshape(-1, 4), want[1]), name
        assert bytes.fromhex(f[nrec]) == want[0].tobytes(), name
