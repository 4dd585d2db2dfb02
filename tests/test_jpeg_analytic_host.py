"""The device JPEG encoder's coefficients against a float64 DCT, without a GPU: tests/jpg_analytic.py (JFIF colour, 2 x 2 mean, level
shift, orthonormal DCT-II, division by the table -- nothing of the encoder's own restatement) holds every quantised coefficient of
every block of the files that the NumPy restatement (jpg_ref.py) and the host build of jpeg_core.hpp (tests/host_jpeg/jpeg_emul.hip)
write, read back by the decoder's restatement.  tests/test_gpu_jpeg_analytic.py does the same for the files the MI355X writes.  The last
tests show that the hold has teeth: encoders that are wrong on purpose fall outside it on the same inputs."""
import functools

import numpy as np
import pytest

import jpg_analytic as A
import jpg_cases as PC
import jpg_ref as R
import sphere_scene
from test_jpeg_device_host import _emul, jpeg_emul  # noqa: F401  (the host build of the product's arithmetic, as that module builds it)

QUALITIES = (1, 50, 95, 100)
SUBSAMPLINGS = ("420", "444")


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def filtered(kind):
    """64 x 96 BGR without one ambiguous sample: 'noise', or 'smooth' = a smooth base perturbed by +-3"""
    return A.cells(64, 96, None if kind == "noise" else PC.smooth(64, 96, 3, 7), seed=11 if kind == "noise" else 12)


@functools.lru_cache(maxsize=None)
def grey_noise():
    return PC.noise(64, 96, 1, 13)


@functools.lru_cache(maxsize=None)
def inputs(subsampling):
    """{label: image}: the filtered images, the SIZES list with 1, 3 and 4 channels and the unfiltered images.  Grey images do not depend
    on the subsampling and are listed under '420' only."""
    out = {"cells_noise": filtered("noise"), "cells_smooth": filtered("smooth")}
    for i, (h, w) in enumerate(PC.SIZES):
        for cn in (1, 3, 4):
            out[f"size_{h}x{w}_cn{cn}"] = (PC.noise if i % 2 else PC.smooth)(h, w, cn, 100 + 10 * i + cn)
    for cn in (1, 3, 4):
        out[f"smooth_cn{cn}"] = PC.smooth(40, 72, cn, 200 + cn)
        out[f"noise_cn{cn}"] = PC.noise(32, 48, cn, 210 + cn)
    out["swing"] = PC.swing()[..., None]
    out["from_coefficients"] = PC.from_coefficients([{16: 1, 33: -1, 51: 1}, {34: 1}, {0: -2, 1: 1, 63: 1}, {63: 2}], 50)[..., None]
    out["sphere"] = np.ascontiguousarray(sphere_scene.render(301)[100:196, 100:196])
    if subsampling != "420":
        out = {k: v for k, v in out.items() if v.shape[2] != 1}
    return out


def check(label, f, bias=False):
    print(A.describe(label, f))
    assert f["excess"] <= 0.0, (label, f)
    if bias:
        assert f["ambiguous"] == 0 and f["bias_n"] >= A.BIAS_MIN_N, (label, f)
        assert abs(f["plain"] - f["plain_expected"]) <= f["plain_limit"], (label, f)
        assert abs(f["signed"] - f["signed_expected"]) <= f["signed_limit"], (label, f)


# ---- the reference itself -------------------------------------------------------------------------------------------------------------
def test_delta_is_derived_and_useful():
    g, m = A.islow_matrices()
    assert np.allclose(g @ g.T, 8 * np.eye(8))                        # a pass is sqrt(8) times an orthonormal transform
    assert np.abs(m - g).max() <= 2.0 * 2.0 ** -14 * 2                # at most a few constants of <= 2^-14 error meet in an entry
    assert set(round(v * 8192) for v in A.ISLOW_13BIT.values()) == {2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172}
    print(f"delta {A.DELTA:.4f} (rounding alone {A.DELTA_ROUNDING:.4f}); table\n{np.array2string(A.DELTA_TABLE, precision=3)}")
    assert A.DELTA_ROUNDING < A.DELTA < 0.5 and A.DELTA_TABLE[0, 0] == 0.0
    assert A.DELTA > 0.175                                            # the largest distance of the restatement from the float64 DCT seen


def test_the_restatements_dct_stays_within_delta_of_the_float64_one():
    """60 000 blocks -- noise, +-full swing, smooth -- before any quantiser: the largest distance, position by position"""
    rng = np.random.default_rng(31)
    y, x = np.mgrid[0:8, 0:8]
    fx, fy, ph, amp = (rng.uniform(lo, hi, (20000, 1, 1)) for lo, hi in ((0, 1.5), (0, 1.5), (0, 6.3), (5, 127)))
    blocks = np.concatenate([rng.integers(0, 256, (20000, 8, 8)), rng.integers(0, 2, (20000, 8, 8)) * 255,
                             np.rint(127.5 + amp * np.sin(fx * x + fy * y + ph)).astype(np.int64)]) - 128
    d = np.abs(R.fdct(blocks) / 8.0 - A.dct(blocks.astype(np.float64)))
    print(f"islow against float64 over {len(blocks)} blocks: largest distance {d.max():.4f} (delta {A.DELTA:.4f}), largest share of "
          f"delta[v, u] {(d.max(0) / np.maximum(A.DELTA_TABLE, 1e-12))[A.DELTA_TABLE > 0].max():.3f}, at delta = 0: {d.max(0)[A.DELTA_TABLE == 0].max():.1e}")
    assert np.all(d <= A.DELTA_TABLE[None] + A.FLOAT_SLACK)
    assert d.max() > 0.5 * A.DELTA_ROUNDING  # (the bound is not idle: rounding alone comes more than half-way to its share)


def test_the_contracts_colour_constants_stay_within_eps_c():
    """INTEGRATION.md section 7, point 2: the largest distance of the 16-bit conversion's argument from the float64 one"""
    real = np.array([[0.299, 0.587, 0.114], [-0.299 / 1.772, -0.587 / 1.772, 0.886 / 1.772], [0.701 / 1.402, -0.587 / 1.402, -0.114 / 1.402]])
    fixed = np.array([[19595, 38470, 7471], [-11059, -21709, 32768], [32768, -27439, -5329]]) / 65536.0
    d = fixed - real
    worst = 255.0 * np.maximum(np.where(d > 0, d, 0).sum(1), np.where(d < 0, -d, 0).sum(1)) + np.array([0, 2.0 ** -16, 2.0 ** -16])
    print("colour constants: largest distance", worst, "EPS_C", A.EPS_C)
    assert worst.max() <= A.EPS_C < 0.01


@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_filtered_images_have_no_ambiguous_sample_and_planes_are_the_rounded_float64_ones(kind):
    img = filtered(kind)
    assert img.shape == (64, 96, 3) and img.dtype == np.uint8
    if kind == "smooth":
        assert np.abs(img.astype(int) - PC.smooth(64, 96, 3, 7)).max() <= 3
    for sub in SUBSAMPLINGS:
        iv = A.sample_intervals(img, sub)
        assert all(np.array_equal(lo, hi) for lo, hi in iv)           # every half-width 0
        want = A.ycc(img)
        if sub == "420":
            want = [want[0]] + [np.rint(p).reshape(32, 2, 48, 2).sum((1, 3)) / 4 for p in want[1:]]
        for got, (lo, _), w in zip(R.planes(img, sub), iv, want):
            assert np.array_equal(got, lo) and np.array_equal(got, np.rint(w))  # (no tie: rint's rule does not matter)


def test_unfiltered_images_do_have_ambiguous_samples():
    """(so the interval form is exercised: chroma sums of 2 (mod 4) are one cell in four)"""
    f = A.hold_file(R.encode(PC.noise(32, 48, 3, 213), 100, "420"), PC.noise(32, 48, 3, 213), 100, "420")
    assert f["ambiguous"] > 100 and "bias_n" not in f


# ---- the restatement and the host build ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("subsampling", SUBSAMPLINGS)
def test_restatement_holds(subsampling, quality):
    worst = -1.0
    for label, img in inputs(subsampling).items():
        f = A.hold_file(R.encode(img, quality, subsampling), img, quality, subsampling)
        if label.startswith("cells"):
            assert f["ambiguous"] == 0
        check(f"restatement {label} {subsampling} q{quality}", f)
        worst = max(worst, f["max"])
    print(f"restatement {subsampling} q{quality}: largest |c q - F| - q / 2 - interval term = {worst:.4f} (delta {A.DELTA:.4f})")


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("subsampling", SUBSAMPLINGS)
def test_host_build_of_jpeg_core_holds(jpeg_emul, subsampling, quality):
    worst = -1.0
    for label, img in inputs(subsampling).items():
        _, _, data = _emul(jpeg_emul, PC.dense(img, quality, subsampling))
        f = A.hold_file(data, img, quality, subsampling)
        check(f"host build {label} {subsampling} q{quality}", f)
        worst = max(worst, f["max"])
    print(f"host build {subsampling} q{quality}: largest |c q - F| - q / 2 - interval term = {worst:.4f} (delta {A.DELTA:.4f})")


def test_host_build_holds_on_a_pitched_window_behind_an_odd_lead(jpeg_emul):
    whole = PC.smooth(48, 128, 3, 90)
    c = PC.window(whole, 31, 45, lead=3, quality=95, subsampling="420", restart=2)
    check("host build window", A.hold_file(_emul(jpeg_emul, c)[2], whole[:, 31:76], 95, "420"))


@pytest.mark.parametrize("subsampling", SUBSAMPLINGS)
def test_bias_at_quality_100(jpeg_emul, subsampling):
    for label, img in (("cells_noise", filtered("noise")), ("grey_noise", grey_noise())):
        check(f"restatement bias {label} {subsampling}", A.hold_file(R.encode(img, 100, subsampling), img, 100, subsampling), bias=True)
        data = _emul(jpeg_emul, PC.dense(img, 100, subsampling))[2]
        check(f"host build bias {label} {subsampling}", A.hold_file(data, img, 100, subsampling), bias=True)


def test_restart_interval_moves_no_coefficient():
    img = filtered("smooth")
    base = A.file_coefficients(R.encode(img, 95, "420"))[0]
    for restart in (1, 4, 65535):
        assert np.array_equal(A.file_coefficients(R.encode(img, 95, "420", restart))[0], base)


# ---- the hold has teeth -----------------------------------------------------------------------------------------------------------------
ISLOW = {"c6": 4433, "c2-c6": 6270, "c2+c6": 15137, "c3": 9633, "t4": 2446, "t5": 16819, "t6": 25172, "t7": 12299, "z1": 7373, "z2": 20995,
         "z3": 16069, "z4": 3196}


def _fdct_pass(d, first, k):
    """jpg_ref._fdct_pass with its constants in a dict, so that one of them can be moved"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[0], out[4] = R._descale(t10 + t11, 2), R._descale(t10 - t11, 2)
    n = 11 if first else 15
    z1 = (t12 + t13) * k["c6"]
    out[2], out[6] = R._descale(z1 + t13 * k["c2-c6"], n), R._descale(z1 - t12 * k["c2+c6"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * k["c3"]
    t4, t5, t6, t7 = t4 * k["t4"], t5 * k["t5"], t6 * k["t6"], t7 * k["t7"]
    z1, z2, z3, z4 = z1 * -k["z1"], z2 * -k["z2"], z3 * -k["z3"] + z5, z4 * -k["z4"] + z5
    out[7], out[5], out[3], out[1] = R._descale(t4 + z1 + z3, n), R._descale(t5 + z2 + z4, n), R._descale(t6 + z2 + z3, n), R._descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def mutant(img, quality, subsampling, mutation=None, constants=None):
    """(coefficients, tables) of an encoder built from the restatement's parts that is wrong in one way: 'transpose', 'swap_chroma',
    'shift_cell' (chroma taken one column to the right), 'truncate', 'half_up' (ties towards plus infinity, not away from zero),
    'luma_table', or ``constants`` for the DCT."""
    a = img if img.ndim == 3 else img[..., None]
    g = R.Geom(a.shape[0], a.shape[1], a.shape[2], subsampling, 1)
    ps = R.planes(a, subsampling)
    if mutation == "swap_chroma":
        ps = [ps[0], ps[2], ps[1]]
    if mutation == "shift_cell":
        ps = [ps[0]] + R.planes(np.concatenate([a[:, 1:], a[:, -1:]], axis=1), subsampling)[1:]
    parts = [R._blocks_of(ps[0], g.mcuy, g.mcux, 2 if g.sub else 1)] + [R._blocks_of(p, g.mcuy, g.mcux, 1) for p in ps[1:]]
    blocks = np.concatenate(parts, axis=2).reshape(-1, 8, 8) - 128
    if mutation == "transpose":
        blocks = blocks.transpose(0, 2, 1)
    k = constants or ISLOW
    d = _fdct_pass(_fdct_pass(blocks.astype(np.int64), True, k).transpose(0, 2, 1), False, k).transpose(0, 2, 1).reshape(-1, 64)
    tabs = A.tables_for(quality, g.nc)
    used = [tabs[0]] * g.nc if mutation == "luma_table" else tabs
    q8 = 8 * np.tile(np.stack(used)[g.comp], (g.nmcu, 1))
    c = np.sign(d) * (np.abs(d) // q8 if mutation == "truncate" else (np.abs(d) + q8 // 2) // q8)
    if mutation == "half_up":
        c = (d + q8 // 2) // q8
    return c[:, R.ZIGZAG], tabs


def _caught(f):
    return f["excess"] > 0.0 or (f.get("bias_n", 0) >= A.BIAS_MIN_N and not A.bias_ok(f))


def test_the_mutant_builder_without_a_mutation_is_the_restatement():
    for sub in SUBSAMPLINGS:
        img = filtered("noise")
        c, tabs = mutant(img, 95, sub)
        assert np.array_equal(c, R.coefficients(img, 95, sub))
        assert not _caught(A.hold(c, tabs, img, sub))


@pytest.mark.parametrize("mutation", ["transpose", "swap_chroma", "shift_cell", "truncate", "half_up", "luma_table"])
def test_wrong_encoders_fall_outside_the_hold(mutation):
    for kind in ("noise", "smooth"):
        img = filtered(kind)
        for sub in SUBSAMPLINGS:
            for q in (50, 100):
                if (mutation == "luma_table" and q == 100) or (mutation == "half_up" and q != 100):
                    continue  # (both tables are all ones there; a tie's direction shows in the bias alone)
                f = A.hold(*mutant(img, q, sub, mutation), img, sub)
                print(A.describe(f"{mutation} {kind} {sub} q{q}", f))
                assert _caught(f), (mutation, kind, sub, q, f)


# jpg_ref._fdct_pass's constant of every jfdctint.c name
NAMES = {"0_298631336": "t4", "0_390180644": "z4", "0_541196100": "c6", "0_765366865": "c2-c6", "0_899976223": "z1", "1_175875602": "c3",
         "1_501321110": "t7", "1_847759065": "c2+c6", "1_961570560": "z3", "2_053119869": "t5", "2_562915447": "z2", "3_072711026": "t6"}


def test_one_dct_constant_off_by_one_unit_falls_outside_the_hold():
    """9633 -> 9634 (FIX(1.175875602), the multiplier of z3 + z4, whose multiplicand is the largest): on ``swing()`` at quality 100 the
    block cut by a horizontal edge has z3 + z4 = 1020 in every row, coefficient (0, 1) moves by 0.125 and one of them sits at a tie.
    That is what the hold can do and no more: a unit moves a coefficient by 0.125 per pass at full swing, below the 0.1875 of rounding
    that delta allows, so of the 24 one-unit changes the hold catches 4 on the inputs of this module (9633 + 1, 16819 + 1, 20995 - 1, 3196 - 1,
    all on ``swing()``); the largest excess is 0.020.  The next test catches all 24."""
    img = PC.swing()[..., None]
    k = dict(ISLOW, c3=ISLOW["c3"] + 1)
    f = A.hold(*mutant(img, 100, "420", None, k), img, "420")
    print(A.describe("9633 + 1, swing q100", f))
    assert f["excess"] > 0.0
    assert A.hold(*mutant(img, 100, "420"), img, "420")["excess"] <= 0.0


@functools.lru_cache(maxsize=None)
def swing_noise():
    return A.swing_noise(88, 128, 21)[..., None]


def _constants_ok(label, est):
    print(f"constants {label}: " + "  ".join(f"{k} {e:+.3f} (+-{lim:.3f})" for k, (e, lim) in est.items()))
    assert all(lim <= 0.5 for _, lim in est.values()), "too few blocks: a unit is not ten standard deviations"
    return all(abs(e) <= lim for e, lim in est.values())


def test_every_dct_constant_is_the_ijg_one_to_half_a_unit(jpeg_emul):
    """the twelve 13-bit constants of the restatement and of the host build of jpeg_core.hpp, estimated from 11 264 full-swing blocks"""
    img = swing_noise()
    assert _constants_ok("restatement", A.constant_estimates(R.coefficients(img, 100), img))
    coef = _emul(jpeg_emul, PC.dense(img, 100))[0]
    assert _constants_ok("host build", A.constant_estimates(coef, img))


@pytest.mark.parametrize("name", list(NAMES))
def test_every_one_unit_change_of_a_dct_constant_is_caught(name):
    img = swing_noise()
    for by in (-1, 1):
        k = dict(ISLOW)
        k[NAMES[name]] += by
        est = A.constant_estimates(mutant(img, 100, "420", None, k)[0], img)
        print(f"{name} {by:+d}: estimated {est[name][0]:+.3f} +- {est[name][1]:.3f}")
        assert abs(est[name][0] - by) <= est[name][1] and abs(est[name][0]) > est[name][1]
