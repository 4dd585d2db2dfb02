"""The two CPU restatements of cv2.remap -- oracle.remap (uint8) and wide_ref.remap (uint16, float32) -- against the float64 analytic
interpolation of tests/analytic_ref.py: kernel shape, anchor, x / y orientation, normalisation, rounding, both saturations and border
folding, within tolerances derived there.  The last tests hold the oracle's output against deliberately wrong references to show that
the same assertions reject them.  tests/test_gpu_analytic.py runs the cases built here through the HIP samplers.

``python tests/test_analytic_remap.py`` prints the measured figures kept in analytic_ref.py (float32 accumulation, signed bias)."""
import sys
from pathlib import Path

import numpy as np
import pytest

import analytic_ref as A
import chainspecs as CS
import wide_ref as W

DTYPES = [np.uint8, np.uint16, np.float32]
BV = {np.uint8: (11, 200, 33), np.uint16: (1000, 60000, 33000), np.float32: (0.25, -0.5, 0.75)}  # (a fourth channel's colour: 0)
SRC_HW = (40, 60)
SMALL_SIZES = [(2, 2), (2, 5), (3, 4), (5, 3), (4, 2), (5, 5)]  # all smaller than the Lanczos footprint: borderInterpolate folds twice
ONE_PIXEL_SIZES = [(1, 4), (3, 1), (1, 1)]  # numpy.pad defines edge, symmetric and wrap on a 1-pixel axis ('reflect' is legacy there)
PLAIN = [("equirect_enc", True), ("poly", [0, 1, -0.1]), CS.EQUI]
ROTATED = [("equirect_enc", True), ("rot", CS.ry(0.3)), ("poly", [0, 1, -0.1]), CS.EQUI]


def restatement(O, dtype):
    """the CPU sampler of a pixel type, as f(src, xm, ym, interp, border, bv)"""
    if np.dtype(dtype) == np.uint8:
        return lambda src, xm, ym, interp, border, bv: O.remap(src, xm, ym, interp, border, bv)
    return lambda src, xm, ym, interp, border, bv: W.remap(src, xm, ym, interp, border, bv)


# ----------------------------------------------------------------------------------------------------------------------- the cases
def noise_case(dtype, cn, interp, seed=0):
    """(src, xm, ym, border, bv): noise, a 200 x 200 map on the 1 / 32 grid from 5 px outside to 5 px inside every edge, BORDER_CONSTANT
    with a colour per channel"""
    src = A.noise(dtype, *SRC_HW, cn, 1000 + seed)
    xm, ym = A.grid_coords(*SRC_HW, 200, 200, 2000 + seed, nearest_safe=interp == A.INTER_NEAREST)
    return src, xm, ym, A.BORDER_CONSTANT, BV[dtype]


def comb_case(dtype, cn, inverse):
    """(src, xm, ym, border, bv): the comb under the sweep of all 1024 fractions at the offsets -4 .. 4 in both axes (288 x 288)"""
    xm, ym = A.sweep_coords()
    return A.comb(*SRC_HW, cn, inverse, dtype), xm, ym, A.BORDER_CONSTANT, 0


def small_border_cases(dtype, border, interp):
    """sources of 2 .. 5 pixels (and of 1 pixel where numpy.pad says what that means), coordinates up to 12 px outside"""
    sizes = SMALL_SIZES + (ONE_PIXEL_SIZES if border != A.BORDER_REFLECT_101 else [])
    for k, (h, w) in enumerate(sizes):
        for cn in ((1, 3, 4)[k % 3],):  # (1, 3 and 4 channels in turn)
            src = A.noise(dtype, h, w, cn, 3000 + 10 * k + cn)
            xm, ym = A.grid_coords(h, w, 32, 48, 4000 + 10 * k + cn, margin=12, nearest_safe=interp == A.INTER_NEAREST)
            yield src, xm, ym, border, 0


WIDE_PLAIN = dict(spec=PLAIN, src_hw=(192, 208), out_wh=(176, 144), radius=96.0, cn=3, border=A.BORDER_CONSTANT)
WIDE_ROT = dict(spec=[("equirect_enc", True), ("rot", CS.ry(0.1)), CS.EQUI], src_hw=(128, 128), out_wh=(120, 112), radius=64.0, cn=4,
                border=A.BORDER_REPLICATE, rots=[CS.ry(a) for a in (0.2, -0.3, 0.05)])


def wide_chain_units(O, geo, dtype):
    """The fused uint16 / float32 cases of tests/test_gpu_analytic.py (the sizes of tests/test_gpu_wide.py): per unit (src, xm, ym,
    border, bv) with the oracle's float32 map of the unit's chain -- one unit, or one per rotation of ``geo['rots']``."""
    for k, rot in enumerate(geo.get("rots", [None])):
        spec = geo["spec"] if rot is None else [geo["spec"][0], ("rot", rot), *geo["spec"][2:]]
        xm, ym = O.get_map(spec, radius=geo["radius"], size_input=geo["src_hw"], size_output=geo["out_wh"])
        yield A.noise(dtype, *geo["src_hw"], geo["cn"], 6000 + k), xm, ym, geo["border"], BV[dtype]


def figures(got, src, xm, ym, interp, border, bv, **kw):
    """analytic_ref.compare at the coordinates the sampler uses: the map itself for NEAREST, its 1 / 32 grid point otherwise"""
    xq, yq, skip = A.quantise(xm, ym)
    if interp == A.INTER_NEAREST:
        xq, yq = np.where(skip, 0, xm).astype(np.float64), np.where(skip, 0, ym).astype(np.float64)
    return A.compare(got, src, xq, yq, interp, border, bv, skip=skip, **kw)


def hold(got, case, interp, label, bias=False):
    """assert one case: every pixel within the tolerance of its type; ``bias``: and the mean deviation within the bias limit"""
    src, xm, ym, border, bv = case
    f = figures(got, src, xm, ym, interp, border, bv)
    print(f"analytic {label}: interp {interp} {got.dtype} max {f['max']:.3g} excess {f['excess']:.3g} bias {f['bias']:+.4f} n {f['n']}")
    assert f["excess"] <= 0.0, (label, interp, f)
    if bias and got.dtype != np.float32 and interp != A.INTER_NEAREST:
        assert f["n"] >= A.BIAS_MIN_SAMPLES, (label, f["n"])
        assert abs(f["bias"]) <= A.bias_limit(got.dtype, interp), (label, interp, f)
    return f


# ----------------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("interp", [0, 1, 2, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_grid_aligned_noise(oracle_mod, dtype, interp):
    run = restatement(oracle_mod, dtype)
    for cn in (1, 3, 4):
        case = noise_case(dtype, cn, interp)
        hold(run(case[0], case[1], case[2], interp, case[3], case[4]), case, interp, f"noise cn{cn}", bias=cn >= 3)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("interp", [1, 2, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_comb_sweep_of_all_fractions(oracle_mod, dtype, interp, inverse):
    run = restatement(oracle_mod, dtype)
    for cn in (1,):  # (the noise cases cover the channel counts; the GPU module sweeps the comb at cn 1, 3 and 4)
        case = comb_case(dtype, cn, inverse)
        got = run(case[0], case[1], case[2], interp, case[3], case[4])
        hold(got, case, interp, f"comb{'-inverse' if inverse else ''} cn{cn}")
        if dtype == np.uint8:  # the sweep did meet both saturations: the comb's negative lobes, the inverse comb's overshoot
            ref = A.sample(case[0], *A.quantise(case[1], case[2])[:2], interp)
            assert interp == 1 or (ref.max() > 255.5 if inverse else ref.min() < -0.5)


@pytest.mark.parametrize("border", [1, 2, 3, 4])
@pytest.mark.parametrize("interp", [0, 1, 2, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_border_modes_on_sources_smaller_than_the_footprint(oracle_mod, dtype, interp, border):
    run = restatement(oracle_mod, dtype)
    n = 0
    for case in small_border_cases(dtype, border, interp):
        hold(run(case[0], case[1], case[2], interp, case[3], case[4]), case, interp, f"border {border} src {case[0].shape}")
        n += 1
    assert n == (6 if border == 4 else 9)


@pytest.mark.parametrize("name,spec", [("plain", PLAIN), ("rotated", ROTATED)])
def test_maps_off_the_grid_through_quantise(oracle_mod, name, spec):
    """Real chain maps do not lie on the 1 / 32 grid: evaluated at quantise()'s grid point the tight tolerance holds all the same."""
    O = oracle_mod
    xm, ym = O.get_map(spec, radius=96.0, size_input=(192, 208), size_output=(256, 256))
    xq, yq, skip = A.quantise(xm, ym)
    assert skip.mean() < 0.01
    assert (np.abs(xm * 32 - np.rint(xm * 32)) > 0.01).mean() > 0.5  # (off the grid indeed)
    for dtype in DTYPES:
        src = A.noise(dtype, 192, 208, 3, 5)
        for interp in (1, 2, 4):
            got = restatement(O, dtype)(src, xm, ym, interp, 0, BV[dtype])
            hold(got, (src, xm, ym, 0, BV[dtype]), interp, f"{name} chain", bias=True)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("geo", [WIDE_PLAIN, WIDE_ROT], ids=["plain", "per_unit_rotation"])
def test_fused_wide_cases_of_the_gpu_module(oracle_mod, geo, dtype):
    """The inputs of the GPU module's fused uint16 / float32 cases through wide_ref: the measured float32 bound holds on them here, so
    a kernel that equals wide_ref byte for byte (tests/test_gpu_wide.py) cannot trip over a rare pixel there."""
    for interp in (1, 2, 4):
        for case in wide_chain_units(oracle_mod, geo, dtype):
            assert A.quantise(case[1], case[2])[2].mean() < 0.01
            hold(W.remap(case[0], case[1], case[2], interp, case[3], case[4]), case, interp, "fused wide")


@pytest.mark.parametrize("padding,border", [("zeros", A.BORDER_CONSTANT), ("border", A.BORDER_REPLICATE)])
def test_bicubic_against_torch_grid_sample(padding, border):
    """A third-party witness: torch's float64 bicubic grid_sample is the same a = -0.75 convolution with the same anchor."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(7)
    h, w = SRC_HW
    src = rng.uniform(-1, 1, (h, w, 3))
    x = rng.uniform(-5, w + 4, (70, 90))
    y = rng.uniform(-5, h + 4, (70, 90))
    x[0, :8], y[0, :8] = np.arange(8), np.arange(8)  # fraction 0 exactly
    grid = torch.from_numpy(np.stack([2 * x / (w - 1) - 1, 2 * y / (h - 1) - 1], -1))[None]
    want = torch.nn.functional.grid_sample(torch.from_numpy(src).permute(2, 0, 1)[None], grid, mode="bicubic", padding_mode=padding,
                                           align_corners=True)[0].permute(1, 2, 0).numpy()
    # (the grid's round trip through [-1, 1] moves a coordinate by ~1e-14; the kernel's slope is below 2 per pixel)
    assert np.abs(A.sample(src, x, y, A.INTER_CUBIC, border, 0) - want).max() < 1e-9


def test_quantise_and_weights_basics():
    xq, yq, skip = A.quantise(np.array([[0.5 / 32, 1.5 / 32, 2.5 / 32, -0.5 / 32, np.nan, 1e30, 7.26]], np.float32),
                              np.zeros((1, 7), np.float32))
    assert xq[0, :4].tolist() == [0.0, 2 / 32, 2 / 32, -0.0] and skip[0].tolist() == [False] * 4 + [True, True, False]
    assert xq[0, 6] == 232 / 32
    f = np.arange(32) / 32.0
    for interp in (1, 2, 4):
        w = A.weights(interp, f)
        assert np.allclose(w.sum(-1), 1.0, atol=1e-15) and w.shape == (32, A.TAPS[interp])
        assert np.allclose(w[0], np.eye(A.TAPS[interp])[A.TAPS[interp] // 2 - 1], atol=1e-15)  # fraction 0: the pixel itself
        assert np.allclose(A.weights(interp, 1 - f[1:]), w[1:, ::-1], atol=1e-15)  # the kernels are even
        # the documented maxima of the uint16 bound (analytic_ref.py) are the ones tolerance() enforces
        worst = float(np.max(A.tolerance(np.uint16, interp, A.sum_abs_weights(f[None, :], f[:, None], interp))))
        assert abs(worst - A.UINT16_MAX_TOL[interp]) < 5e-4, (interp, worst)


# ----------------------------------------------------------------------------------------------------------------------- teeth
MUTANTS = [("a=-0.5", 2), ("lanczos3", 4), ("swap", 2), ("swap", 4), ("swap", 1), ("anchor", 1), ("anchor", 2), ("anchor", 4)]


@pytest.mark.parametrize("mutation,interp", MUTANTS)
def test_teeth_a_wrong_reference_is_rejected_by_a_wide_margin(oracle_mod, mutation, interp):
    """oracle.remap's comb sweep held against a reference with another cubic, another window, the axes' weights swapped or the footprint
    one tap off: 8 LSB and more beyond the tolerance that the right reference meets."""
    case = comb_case(np.uint8, 1, False)
    src, xm, ym, border, bv = case
    got = oracle_mod.remap(src, xm, ym, interp, border, bv)
    assert figures(got, src, xm, ym, interp, border, bv)["excess"] <= 0.0
    f = figures(got, src, xm, ym, interp, border, bv, mutation=mutation)
    print(f"teeth {mutation} interp {interp}: max {f['max']:.2f} excess {f['excess']:.2f} bad {f['bad']}")
    assert f["excess"] > 8.0, f


@pytest.mark.parametrize("interp", [1, 2, 4])
def test_teeth_a_floor_in_place_of_the_rounding_is_rejected(oracle_mod, interp):
    """A reference that truncates: the tolerance breaks on the comb (by little: rounding and truncation differ by half an LSB), and the
    signed bias of a noise case sits at +0.5, ten times its limit."""
    src, xm, ym, border, bv = comb_case(np.uint8, 1, False)
    got = oracle_mod.remap(src, xm, ym, interp, border, bv)
    f = figures(got, src, xm, ym, interp, border, bv, floor=True)
    assert f["excess"] > 0.0, f
    src, xm, ym, border, bv = noise_case(np.uint8, 3, interp)
    got = oracle_mod.remap(src, xm, ym, interp, border, bv)
    f = figures(got, src, xm, ym, interp, border, bv, floor=True)
    print(f"teeth floor interp {interp}: bias {f['bias']:+.3f} excess {f['excess']:.3f}")
    assert f["bias"] > 0.4 and f["bias"] > 8 * A.bias_limit(np.uint8, interp), f


# ----------------------------------------------------------------------------------------------------------------------- measurement
def measure(O, seeds=range(8)):
    """The measured constants of analytic_ref.py, from the CPU restatements on the grid-aligned noise cases (cn = 3)."""
    for interp in (1, 2, 4):
        rel, peak, bias = 0.0, 0.0, {np.uint8: 0.0, np.uint16: 0.0}
        absmax = 0.0
        for seed in seeds:
            for dtype in DTYPES:
                src, xm, ym, border, bv = noise_case(dtype, 3, interp, seed)
                got = restatement(O, dtype)(src, xm, ym, interp, border, bv)
                xq, yq, _ = A.quantise(xm, ym)
                ref, aw, awp, pk = A.sample(src, xq, yq, interp, border, bv, with_abs=True)
                d = got.astype(np.float64) - A.expected(dtype, ref)
                if dtype == np.float32:
                    rel = max(rel, float((np.abs(d) / awp).max()))
                    peak = max(peak, float((np.abs(d) / (aw[..., None] * pk)).max()))
                    absmax = max(absmax, float(np.abs(d).max()))
                else:
                    bias[dtype] = max(bias[dtype], abs(float(d.mean())))
                    print(f"  interp {interp} {np.dtype(dtype).name} seed {seed}: max {np.abs(d).max():.4f} mean {d.mean():+.5f}")
        print(f"interp {interp}: float32 max |d| / sum|w p| = {rel:.3e}, / (sum|w| max|p|) = {peak:.3e} (max |d| {absmax:.3e}); largest |bias| uint8 {bias[np.uint8]:.5f} "
              f"uint16 {bias[np.uint16]:.5f}")


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    from oracle import oracle as _O

    _O.build()
    measure(_O)
