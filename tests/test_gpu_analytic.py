"""The HIP samplers on the MI355X against the float64 analytic interpolation of tests/analytic_ref.py -- directly, not through the
oracle's restatement of cv2.remap: kernel shape, anchor, x / y orientation, normalisation, rounding, saturation and border folding of
every kernel family, within the tolerances derived in analytic_ref.py.  The oracle supplies only the float32 coordinate maps of the
fused chains (pinned against the reference's goldens; the device reproduces them bucket for bucket, tests/test_gpu_parity.py), which
``quantise`` takes to the 1 / 32 grid point the sampler uses.

Every case asserts the kernel family that served it (``last_launch_kinds``; the two C ABI entry points that sample a caller's map ARE
their kernel: v1c_remap_lut = k_remap 'generic', v1c_remap_lut_ex = k_remap_wide 'wide'), and the last test checks that between them
the cases reached every family.  Outputs larger than 300 x 300 are held to the reference on a fixed seeded eighth of their pixels, all
of the last (ragged) tile row and tile column, and both rows at the mirror line."""
import numpy as np
import pytest
import torch

import analytic_ref as A
import chainspecs as CS
import test_analytic_remap as T
from test_gpu_parity import LEAN_BATCH, MIRROR_GEOMETRIES
from test_gpu_round5 import KXK_EDGE_CASES

pytestmark = pytest.mark.gpu

DEPTH = {np.uint16: 2, np.float32: 5}
EQUI = [("equirect_enc", True), CS.EQUI]
_REACHED: set = set()  # kernel families the cases of this module were served by
WANTED = {"generic", "wide", "tile/K4", "tile/K8", "kxk-auto", "cn", "mirror", "batch", "rot_pair"}
# What the launch reports is the family ('tile', 'cn', ...).  Three entries are finer than that and rest on the dispatcher: 'tile/K4' and
# 'tile/K8' are a 'tile' launch with INTER_CUBIC / INTER_LANCZOS4 (the kernel's K is a template argument chosen from the interpolation),
# 'kxk-auto' is a 'tile' launch of a K x K pair in the device form of radius="auto" (last_auto_radius_form() == 'device': the launch
# without plan-time boxes).  Nothing observable tells them apart beyond that, as in tests/test_gpu_auto_radius.py and test_gpu_round5.py.


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


# ----------------------------------------------------------------------------------------------------------------------- helpers
def lut(R, dev, case, interp):
    """one (src, xm, ym, border, bv) case through v1c_remap_lut (uint8) / v1c_remap_lut_ex (uint16, float32): the output image"""
    from vr180_convert_amd import _native

    src, xm, ym, border, bv = case
    hs, ws, cn = src.shape
    ho, wo = xm.shape
    s_d, x_d, y_d = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (src, xm, ym))
    out = torch.zeros((ho, wo, cn), dtype=s_d.dtype, device=dev)
    isz = src.dtype.itemsize
    lib = _native.lib()
    if src.dtype == np.uint8:
        cv = R.border_scalar(bv)
        rc = lib.v1c_remap_lut(dev.index, R._stream_ptr(dev), s_d.data_ptr(), hs, ws, ws * cn, cn, out.data_ptr(), ho, wo, wo * cn,
                               x_d.data_ptr(), y_d.data_ptr(), wo * 4, interp, border, cv.ctypes.data)
        _native.check(rc, "v1c_remap_lut")
        _REACHED.add("generic")
    else:
        cv = R.border_scalar_f64(bv)
        rc = lib.v1c_remap_lut_ex(dev.index, R._stream_ptr(dev), s_d.data_ptr(), hs, ws, ws * cn * isz, cn, DEPTH[src.dtype.type],
                                  out.data_ptr(), ho, wo, wo * cn * isz, x_d.data_ptr(), y_d.data_ptr(), wo * 4, interp, border,
                                  cv.ctypes.data)
        _native.check(rc, "v1c_remap_lut_ex")
        _REACHED.add("wide")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def pick(ho, wo, mirror=False):
    """the pixels of an output that are held to the reference: all of them up to 300 x 300, else a seeded eighth, the last 32 rows and
    64 columns or what is left of them (the ragged tile row and column) and the two rows at the mirror line"""
    if ho * wo <= 300 * 300:
        return np.ones((ho, wo), bool)
    m = np.random.default_rng(10007 * ho + wo).random((ho, wo)) < 0.125
    m[ho - (ho % 32 or 32):] = True
    m[:, wo - (wo % 64 or 64):] = True
    if mirror:
        m[ho // 2 - 1:ho // 2 + 1] = True
    return m


def hold_fused(O, got, src, spec, *, radius, out_wh, interp, border, bv, label, mirror=False, bias=False):
    """one unit of a fused launch against sample(src, *quantise(O.get_map(...)), ...)"""
    xm, ym = O.get_map(spec, radius=radius, size_input=src.shape[:2], size_output=out_wh)
    xq, yq, skip = A.quantise(xm, ym)
    assert skip.mean() < 0.01, (label, float(skip.mean()))
    sel = pick(out_wh[1], out_wh[0], mirror)
    f = A.compare(got[sel], src, xq[sel], yq[sel], interp, border, bv, skip=skip[sel])
    print(f"analytic {label}: interp {interp} {got.dtype} max {f['max']:.3g} excess {f['excess']:.3g} bias {f['bias']:+.4f} n {f['n']}")
    assert f["excess"] <= 0.0, (label, interp, f)
    if bias and got.dtype != np.float32:
        assert f["n"] >= A.BIAS_MIN_SAMPLES, (label, f["n"])
        assert abs(f["bias"]) <= A.bias_limit(got.dtype, interp), (label, interp, f)


def sources(kind, h, w, cn, n, seed):
    """n sources of one kind: 'noise', or 'comb' = the comb and its inverse in turn (lattice phases differ from unit to unit)"""
    if kind == "noise":
        return [A.noise(np.uint8, h, w, cn, seed + k) for k in range(n)]
    return [A.comb(h, w, cn, inverse=k % 2 == 1, phase=(k % 5, (3 * k) % 7)) for k in range(n)]


def run_units(V, R, dev, spec, imgs, out_wh, *, radius, interp, border=0, bv=0, rotations=None):
    srcs = [torch.from_numpy(i).to(dev) for i in imgs]
    dsts = [torch.full((out_wh[1], out_wh[0], imgs[0].shape[2]), 99, dtype=srcs[0].dtype, device=dev) for _ in imgs]
    assert V.remap_tensors(CS.to_product(spec), srcs, dsts, radius=radius, interpolation=interp, boarder_mode=border, boarder_value=bv,
                           rotations=rotations) == ["ray"]
    torch.cuda.synchronize()
    return [d.cpu().numpy() for d in dsts], R.last_launch_kinds()


# ----------------------------------------------------------------------------------------------------------------------- caller's maps
@pytest.mark.parametrize("interp", [0, 1, 2, 4])
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_lut_grid_aligned_noise(R, dev, dtype, interp):
    for cn in (1, 3, 4):
        case = T.noise_case(dtype, cn, interp)
        T.hold(lut(R, dev, case, interp), case, interp, f"lut noise cn{cn}", bias=cn >= 3)


@pytest.mark.parametrize("interp", [1, 2, 4])
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_lut_comb_sweep_of_all_fractions(R, dev, dtype, interp):
    """one launch per interpolation and source: all 1024 fractions at the offsets -4 .. 4 in both axes, stacked into one 288 x 288 map"""
    for inverse in (False, True):
        for cn in ((1, 3, 4) if dtype == np.uint8 else (1,)):
            case = T.comb_case(dtype, cn, inverse)
            T.hold(lut(R, dev, case, interp), case, interp, f"lut comb{'-inverse' if inverse else ''} cn{cn}")


@pytest.mark.parametrize("border", [1, 2, 3, 4])
@pytest.mark.parametrize("interp", [0, 1, 2, 4])
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_lut_border_modes_on_sources_smaller_than_the_footprint(R, dev, dtype, interp, border):
    for case in T.small_border_cases(dtype, border, interp):
        T.hold(lut(R, dev, case, interp), case, interp, f"lut border {border} src {case[0].shape}")


# ----------------------------------------------------------------------------------------------------------------------- fused, BGR K x K
C0 = (EQUI, (256, 256), (256, 256), 128.0, 0)  # the reference's own test size: radius "max", black border
KXK = {
    # name: ((spec, source (H, W), output (W, H), radius, border value), border mode)
    "c0": (C0, 0),
    "edge_constant": (KXK_EDGE_CASES["circle_beyond_the_frame"], 0),
    "edge_replicate": (KXK_EDGE_CASES["circle_beyond_the_frame"], 1),
    "edge_reflect_101": (KXK_EDGE_CASES["circle_beyond_the_frame"], 4),
    "rotated": (KXK_EDGE_CASES["rotated"], 0),
}


@pytest.mark.parametrize("kind", ["noise", "comb"])
@pytest.mark.parametrize("interp", [2, 4])
@pytest.mark.parametrize("name", list(KXK))
def test_fused_kxk_pairs_on_bgr(V, R, oracle_mod, dev, name, interp, kind):
    """k_ray_lin3_tile with 4 x 4 and 8 x 8 taps: pairs, footprints inside the source and across its frame under a three-component
    border colour, REPLICATE and REFLECT_101, and a rotated chain"""
    (spec, (hs, ws), out_wh, radius, bv), border = KXK[name]
    imgs = sources(kind, hs, ws, 3, 2, 100)
    got, kinds = run_units(V, R, dev, spec, imgs, out_wh, radius=radius, interp=interp, border=border, bv=bv)
    assert kinds == ["tile"], (name, interp, kinds)
    _REACHED.add("tile/K4" if interp == 2 else "tile/K8")
    for k in range(2):
        hold_fused(oracle_mod, got[k], imgs[k], spec, radius=radius, out_wh=out_wh, interp=interp, border=border, bv=bv,
                   label=f"kxk {name} {kind} {k}", bias=kind == "noise")


def _disc(img, r, cx=None):
    h, w = img.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    out = img.copy()
    out[(xx - (w / 2 if cx is None else cx)) ** 2 + (yy - h / 2) ** 2 > r * r] = 0
    return out


@pytest.mark.parametrize("kind", ["noise", "comb"])
@pytest.mark.parametrize("interp", [2, 4])
def test_box_less_kxk_pair_with_the_radius_found_on_the_device(V, R, oracle_mod, dev, interp, kind):
    """k_ray_kxk_auto_pair through apply_lr_tensors(radius="auto"): image circles on black (the estimate needs them), the smallest
    geometry of tests/test_gpu_auto_radius.py.  The comb's run uses the inverse comb (dots on white: a circle get_radius can find)."""
    O = oracle_mod
    spec = [("equirect_enc", True), ("poly", [0, 1, -0.05]), CS.EQUI]
    full = [np.maximum(A.noise(np.uint8, 360, 360, 3, 300 + k), 40) for k in range(2)] if kind == "noise" else \
        [A.comb(360, 360, 3, inverse=True, phase=(k, 2 * k)) for k in range(2)]
    imgs = [_disc(full[0], 170), _disc(full[1], 158.5, cx=176)]
    radius = max(O.get_radius(im) for im in imgs)
    got = V.apply_lr_tensors(CS.to_product(spec), torch.from_numpy(imgs[0]).to(dev), torch.from_numpy(imgs[1]).to(dev),
                             size_output=(288, 288), interpolation=interp, boarder_value=(17, 200, 90), radius="auto",
                             auto_radius_on_device=True).cpu().numpy()
    assert R.last_auto_radius_form() == "device" and R.last_launch_kinds() == ["tile"], (R.last_auto_radius_form(), R.last_launch_kinds())
    _REACHED.add("kxk-auto")
    for k in range(2):
        hold_fused(O, got[:, 288 * k:288 * (k + 1)], imgs[k], spec, radius=radius, out_wh=(288, 288), interp=interp, border=0,
                   bv=(17, 200, 90), label=f"kxk-auto {kind} {k}")


# ----------------------------------------------------------------------------------------------------------------------- gray, BGRA
@pytest.mark.parametrize("cn", [1, 4])
@pytest.mark.parametrize("interp", [1, 2, 4])
def test_gray_and_bgra_comb_through_the_cn_kernel(V, R, oracle_mod, dev, interp, cn):
    """k_ray_lin_cn at 613 x 587: comb sources with the same values in every channel, so alpha is held to the weights of the others"""
    imgs = sources("comb", 300, 320, cn, 2, 0)
    got, kinds = run_units(V, R, dev, EQUI, imgs, (613, 587), radius=140.0, interp=interp, border=0, bv=77)
    assert kinds == ["cn"], (interp, cn, kinds)
    _REACHED.add("cn")
    for k in range(2):
        hold_fused(oracle_mod, got[k], imgs[k], EQUI, radius=140.0, out_wh=(613, 587), interp=interp, border=0, bv=77,
                   label=f"cn{cn} comb {k}")
        if cn == 4:
            assert np.array_equal(got[k][..., 3], got[k][..., 1]) and np.array_equal(got[k][..., 3], got[k][..., 2])


# ----------------------------------------------------------------------------------------------------------------------- bilinear DMA kernels
# (these compute bilinear as a dot product of 10-bit weight pairs, not from the table: another statement of the same arithmetic)
@pytest.mark.parametrize("kind", ["noise", "comb"])
def test_bilinear_mirror_pair_and_single_image(V, R, oracle_mod, dev, kind):
    (hs, ws), out_wh, radius, kind_m, _ = MIRROR_GEOMETRIES[0]
    assert kind_m == "mirror"
    imgs = sources(kind, hs, ws, 3, 2, 400)
    got = V.apply_lr_tensors(CS.to_product(EQUI), torch.from_numpy(imgs[0]).to(dev), torch.from_numpy(imgs[1]).to(dev),
                             size_output=out_wh, interpolation=1, radius=radius, boarder_value=(5, 6, 7)).cpu().numpy()
    assert R.last_launch_kinds() == ["mirror"], R.last_launch_kinds()
    for k in range(2):
        hold_fused(oracle_mod, got[:, out_wh[0] * k:out_wh[0] * (k + 1)], imgs[k], EQUI, radius=radius, out_wh=out_wh, interp=1, border=0,
                   bv=(5, 6, 7), label=f"mirror pair {kind} {k}", mirror=True, bias=kind == "noise")
    one, kinds = run_units(V, R, dev, EQUI, imgs[1:], out_wh, radius=radius, interp=1, bv=(5, 6, 7))
    assert kinds == ["mirror"], kinds
    _REACHED.add("mirror")
    hold_fused(oracle_mod, one[0], imgs[1], EQUI, radius=radius, out_wh=out_wh, interp=1, border=0, bv=(5, 6, 7),
               label=f"mirror single {kind}", mirror=True, bias=kind == "noise")


@pytest.mark.parametrize("kind", ["noise", "comb"])
def test_bilinear_lean_batch_with_rest_tiles(V, R, oracle_mod, dev, kind):
    """k_ray_lin3_batch_lean_raw: 11 units sharing the map (workgroups of 8 + 3), its rest tiles in the pair kernel"""
    (hs, ws), out_wh, spec, radius = LEAN_BATCH["m_table"]
    imgs = sources(kind, hs, ws, 3, 11, 500)
    got, kinds = run_units(V, R, dev, spec, imgs, out_wh, radius=radius, interp=1, bv=(5, 6, 7))
    assert kinds == ["batch"], kinds
    _REACHED.add("batch")
    for k in (0, 7, 8, 10):
        hold_fused(oracle_mod, got[k], imgs[k], spec, radius=radius, out_wh=out_wh, interp=1, border=0, bv=(5, 6, 7),
                   label=f"batch {kind} {k}", bias=kind == "noise")


@pytest.mark.parametrize("kind", ["noise", "comb"])
def test_bilinear_units_with_a_rotation_each(V, R, oracle_mod, dev, kind):
    """k_ray_lin3_rot_pair_raw: units overriding the chain's rotation, three of them (the second pair half empty).  No ROT_UNITS geometry
    reaches it -- the kernel wants rays close enough for one table entry per lane, outputs from ~416 px on; theirs stay in the general
    tile kernel -- so this is the 160 x 160 -> 448 x 448 geometry of test_more_units_than_a_ring_slot_holds, which asserts the family."""
    (hs, ws), out_wh, radius = (160, 160), (448, 448), 80.0
    specs = [CS.c5_spec(f // 2, f % 2) for f in range(3)]
    imgs = sources(kind, hs, ws, 3, 3, 600)
    base = [("equirect_enc", True), ("rot_quat", (1.0, 0.0, 0.0, 0.0)), CS.EQUI]
    got, kinds = run_units(V, R, dev, base, imgs, out_wh, radius=radius, interp=1, bv=(1, 2, 3), rotations=[s[1][1] for s in specs])
    assert kinds == ["rot_pair"], kinds
    _REACHED.add("rot_pair")
    for k, spec in enumerate(specs):
        hold_fused(oracle_mod, got[k], imgs[k], spec, radius=radius, out_wh=out_wh, interp=1, border=0, bv=(1, 2, 3),
                   label=f"rot_pair {kind} {k}", bias=kind == "noise")


# ----------------------------------------------------------------------------------------------------------------------- fused, wide
@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("geo", [T.WIDE_PLAIN, T.WIDE_ROT], ids=["plain", "per_unit_rotation"])
def test_fused_chains_on_uint16_and_float32(V, R, oracle_mod, dev, geo, dtype):
    """k_remap_wide behind a lowered chain: one plain chain, one with a rotation per unit (tests/test_analytic_remap.py runs the same
    inputs through wide_ref)"""
    for interp in (1, 2, 4):
        cases = list(T.wide_chain_units(oracle_mod, geo, dtype))
        srcs = [torch.from_numpy(c[0]).to(dev) for c in cases]
        dsts = [torch.zeros((geo["out_wh"][1], geo["out_wh"][0], geo["cn"]), dtype=srcs[0].dtype, device=dev) for _ in cases]
        rots = [np.array(r) for r in geo["rots"]] if "rots" in geo else None
        V.remap_tensors(CS.to_product(geo["spec"]), srcs, dsts, radius=geo["radius"], interpolation=interp, boarder_mode=geo["border"],
                        boarder_value=T.BV[dtype], rotations=rots)
        torch.cuda.synchronize()
        kinds = R.last_launch_kinds()
        assert kinds and all(k in ("wide", "wide+fixup") for k in kinds), kinds
        _REACHED.add("wide")
        for case, d in zip(cases, dsts):
            assert A.quantise(case[1], case[2])[2].mean() < 0.01
            T.hold(d.cpu().numpy(), case, interp, f"fused wide {np.dtype(dtype).name}")


def test_the_cases_reached_every_kernel_family():
    """(the tests above ran: each records the family its launch reported)"""
    assert WANTED <= _REACHED, sorted(WANTED - _REACHED)
