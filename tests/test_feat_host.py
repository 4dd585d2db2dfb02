"""Feature matching (--automatch devfm) without a GPU: the NumPy restatement's own sanity, the product's feat_core.hpp arithmetic run on
the host against it, the sampling pattern, the C ABI's argument checks, the resource budget of kernels_feat.o and the CLI glue."""
import ctypes as C
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import feat_ref as R

ROOT = Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "host_feat" / "feat_emul.hip"


@pytest.fixture(scope="module")
def feat_emul(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_feat") / "libfeat_emul.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-fno-fast-math", "-o", str(out),
                    str(HARNESS)], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(out))
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    lib.feat_resample.argtypes = [vp, i32, i32, i64, i32, vp, vp, i32, i32, vp]
    lib.feat_smooth.argtypes = [vp, i32, i32, vp]
    lib.feat_fast.argtypes = [vp, i32, i32, vp]
    lib.feat_nms.argtypes = [vp, i32, i32, vp]
    lib.feat_orient.argtypes = [vp, i32, vp, i32, vp, vp]
    lib.feat_best.argtypes = [vp, i32, vp, i32, i32, vp]
    return lib


def _ptr(a):
    return a.ctypes.data


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_fast_fires_at_polygon_vertices_not_on_edges():
    img = np.full((96, 96), 40, np.uint8)
    img[20:60, 30:70] = 200  # an axis-aligned rectangle: four corners, four straight edges
    sc = R.fast_scores(img)
    ys, xs = R.nms(np.where(sc >= 20, sc, 0).astype(np.uint8))
    corners = {(20, 30), (20, 69), (59, 30), (59, 69)}
    found = set(zip(ys.tolist(), xs.tolist()))
    assert all(min(abs(y - cy) + abs(x - cx) for cy, cx in corners) <= 2 for y, x in found), found
    assert all(any(abs(y - cy) + abs(x - cx) <= 2 for y, x in found) for cy, cx in corners), found
    assert sc[40, 30] < 20 and sc[20, 50] < 20 and sc[40, 69] < 20  # middles of the edges: no score


def test_blob_direction_selects_the_sector():
    yy, xx = np.mgrid[-40:41, -40:41].astype(float)
    for k in range(R.BINS):
        th = math.radians(12 * k + 6)
        blob = 200 * np.exp(-((xx - 8 * math.cos(th)) ** 2 + (yy - 8 * math.sin(th)) ** 2) / 12) + 20
        sm = blob.round().astype(np.uint8)
        m10, m01 = R.moments(sm, np.array([40]), np.array([40]))
        assert R.orient_bins(m10, m01)[0] == k, k
    assert R.orient_bins(np.array([0]), np.array([0]))[0] == 0


def test_pattern_is_256_pairs_inside_the_disc_and_deterministic():
    p = R.pattern()
    assert p.shape == (30, 256, 4)
    assert ((p[..., 0].astype(int) ** 2 + p[..., 1].astype(int) ** 2) <= 15 * 15).all()
    assert ((p[..., 2].astype(int) ** 2 + p[..., 3].astype(int) ** 2) <= 15 * 15).all()
    assert np.array_equal(p, R.pattern())
    b = R.base_pattern()
    assert 4.5 < b.std() < 7 and len({tuple(r) for r in b.tolist()}) == 256


def test_restated_matcher_equals_plain_brute_force():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, (60, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (50, 32), dtype=np.uint8)
    b[10], b[20] = a[3], a[3]          # two candidates at distance 0: the tie goes to the lower index (0 <= 3/4 * 0 passes)
    b[30] = a[5]
    b[31] = a[5] ^ 1                   # best 0, second 1
    a[40] = b[7]
    a[41] = b[7]                       # b[7]'s best is a[40]: a[41] is not mutual
    for ratio, dmax in (((3, 4), 64), ((1, 1), 256), ((3, 4), 90)):
        got = R.match(a, b, max_distance=dmax, ratio=ratio)
        want = []
        for i in range(len(a)):
            d = [sum(bin(int(x)).count("1") for x in (a[i] ^ b[j])) for j in range(len(b))]
            j = min(range(len(b)), key=lambda k: (d[k], k))
            d2 = sorted(d)[1]
            dt = [sum(bin(int(x)).count("1") for x in (a[k] ^ b[j])) for k in range(len(a))]
            back = min(range(len(a)), key=lambda k: (dt[k], k))
            if back == i and d[j] <= dmax and ratio[1] * d[j] <= ratio[0] * d2:
                want.append((i, j, d[j]))
        assert [tuple(map(int, t)) for t in zip(*got)] == want, ratio
    i1, i2, _ = R.match(a, b)
    assert (3, 10) in zip(i1.tolist(), i2.tolist()) and (5, 30) in zip(i1.tolist(), i2.tolist()) and (40, 7) in zip(i1.tolist(), i2.tolist())


def _tied_sets(seed, na, nb):
    """random descriptors with near copies, exact duplicates on both sides and tied non-zero distances"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (na, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    if nb > 40:
        k = na // 3
        a[:k] = b[rng.integers(0, nb, k)] ^ rng.integers(0, 2, (k, 32), dtype=np.uint8)
        b[10] = b[20] = b[nb - 1] = a[na - 1]       # three candidates at distance 0 of one query, the last index among them
        b[30] = b[31] = a[na - 2] ^ 1               # a tied non-zero best
        if na > 40:
            a[5] = a[6] = a[na // 2] = b[3]         # ... and duplicates among the queries: ties of the columns
    return a, b


@pytest.mark.parametrize("na,nb", [(300, 211), (211, 300), (257, 1), (1, 257), (64, 64)])
def test_blocked_matcher_equals_the_unblocked_one(na, nb):
    """feat_ref.match_blocked (rows a block at a time, a running best / lowest index / second best of every column) against
    feat_ref.match on one matrix: blocks of 1, 7 and 100 rows and a single block, nb == 1 (NO_SECOND), exact duplicates, every ratio and
    max_distance the GPU fuzz draws; and the column results, which serve the swapped argument order"""
    a, b = _tied_sets(na * 1000 + nb, na, nb)
    d = R.distances(a, b)
    for rows in (1, 7, 100, na):
        got_rows, got_cols = R.best_both(a, b, block_bytes=rows * 4 * nb)
        assert all(np.array_equal(g, w) for g, w in zip(got_rows, R.best(d))), rows
        assert all(np.array_equal(g, w) for g, w in zip(got_cols, R.best(d.T))), rows
    assert np.array_equal(d, R.distances(a, b))
    if nb == 1:
        assert (got_rows[2] == R.NO_SECOND).all()
    n_kept = 0
    for dmax in (0, 16, 64, 256):
        for ratio in ((3, 4), (1, 1), (1, 2), (0, 1)):
            want = R.match(a, b, max_distance=dmax, ratio=ratio)
            got = R.match_blocked(a, b, max_distance=dmax, ratio=ratio, block_bytes=7 * 4 * nb)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (dmax, ratio)
            back = R.match_from_best(got_cols, got_rows, dmax, ratio)
            assert all(np.array_equal(g, w) for g, w in zip(back, R.match(b, a, max_distance=dmax, ratio=ratio))), (dmax, ratio)
            n_kept += len(want[0])
    assert n_kept > 0
    for x, y in ((a[:0], b), (a, b[:0])):
        assert all(len(v) == 0 for v in R.match_blocked(x, y))


def test_radius_helper_hands_the_magnitude_of_the_auto_radius_to_the_detector(product_lib):
    """radius="auto" on an image circle on black is negative (the reference's sign quirk, kept); v1c_feat_detect refuses radius <= 0, so
    features.resolve_radius gives its magnitude -- for one image and for a pair -- and leaves "max" and numbers alone."""
    from vr180_convert_amd import features as F
    from vr180_convert_amd.chain import get_radius
    from vr180_convert_amd.remapper import get_radius_smart

    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[:480, :640]
    disc = rng.integers(30, 256, (480, 640, 3), dtype=np.uint8)
    disc[(xx - 320) ** 2 + (yy - 240) ** 2 > 200 ** 2] = 0
    yy, xx = np.mgrid[:512, :512]
    disc2 = rng.integers(30, 256, (512, 512, 3), dtype=np.uint8)
    disc2[(xx - 256) ** 2 + (yy - 256) ** 2 > 230 ** 2] = 0
    assert get_radius(disc) == -200.5 and get_radius(disc2) == -230.5
    assert F.resolve_radius("auto", [disc]) == 200.5 == -get_radius(disc)
    assert F.resolve_radius("auto", [disc, disc2]) == abs(get_radius_smart("auto", [disc, disc2])) == 200.5
    assert F.resolve_radius("max", [disc]) == 240.0 and F.resolve_radius(123.25, [disc]) == 123.25
    assert F.params(1.0, F.resolve_radius("auto", [disc])).radius > 0
    # what the detector answered to the raw value (before any device call): the refusal that `lr --automatch devfm` ended in
    buf, prm = np.zeros(1 << 16, np.uint8), F.params(1.0, get_radius_smart("auto", [disc]))
    assert product_lib.v1c_feat_detect(0, None, _ptr(buf), 480, 640, 640 * 3, 3, C.byref(prm), _ptr(buf), _ptr(buf), _ptr(buf)) == -1
    assert "radius must lie in (0, 1e9]" in product_lib.v1c_last_error().decode()
    with pytest.raises(IndexError):  # no black border: what the reference's match_lr raises too
        F.resolve_radius("auto", [rng.integers(30, 256, (64, 64, 3), dtype=np.uint8)])


def test_feat_fuzz_draws_few_cases_that_the_detector_refuses():
    """tools/fuzz.py --feat draws sizes, scales, radii and margins so that v1c_feat_detect refuses a small minority (a working image under
    33 x 33, an empty circle): feat_ref.refusal over 3000 draws of the seed the GPU suite runs stays under 8 % -- the GPU slice fails
    above 10 % --, both reasons occur, and the predicate agrees with the library's own argument checks (which run before any device call)."""
    import importlib.util

    from vr180_convert_amd import _native
    from vr180_convert_amd import features as F

    sp = importlib.util.spec_from_file_location("v1c_fuzz_tool", ROOT / "tools" / "fuzz.py")
    Z = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(Z)
    lib = _native.lib()
    buf = np.zeros(700 * 700 * 4 + 64, np.uint8)  # stands in for the device image: a refusal comes before any device call
    why = {}
    for case in range(3000):
        rng = np.random.default_rng([203, case])
        rng.random()
        p = Z.feat_draw(rng)
        r = R.refusal(p["h"], p["w"], p["scale"], p["radius"], p["margin"])
        why[r] = why.get(r, 0) + 1
        if r is not None:
            prm = F.params(p["scale"], p["radius"], margin=p["margin"])
            rc = lib.v1c_feat_detect(0, None, _ptr(buf), p["h"], p["w"], p["w"] * p["cn"], p["cn"], C.byref(prm), _ptr(buf), _ptr(buf), _ptr(buf))
            assert rc == -1 and any(t in lib.v1c_last_error().decode() for t in ("smaller than the pattern", "empty circle", "empty source")), (p, r)
    print(why)
    refused = 3000 - why.get(None, 0)
    assert 0 < refused <= 0.08 * 3000, why
    assert why.get("working image under 33 x 33", 0) > 0 and why.get("empty circle", 0) > 0, why


# ---- the product's arithmetic on the host -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn,s", [(1, 1.0), (3, 0.5), (4, 0.37), (3, 0.25)])
def test_host_harness_equals_restatement_per_pixel(feat_emul, cn, s):
    rng = np.random.default_rng(cn * 100 + int(s * 100))
    h, w = 203, 257
    img = rng.integers(0, 256, (h, w, cn), dtype=np.uint8)
    img[40:120, 50:150] //= 3
    y, rb, cb = R.resample(img, s)
    got = np.zeros_like(y)
    r32, c32 = rb.astype(np.int32), cb.astype(np.int32)
    feat_emul.feat_resample(_ptr(img), h, w, w * cn, cn, _ptr(r32), _ptr(c32), y.shape[0], y.shape[1], _ptr(got))
    assert np.array_equal(got, y)
    sm = np.zeros_like(y)
    feat_emul.feat_smooth(_ptr(np.ascontiguousarray(y)), y.shape[0], y.shape[1], _ptr(sm))
    assert np.array_equal(sm, R.smooth(y))
    fs = np.zeros(y.shape, np.int32)
    feat_emul.feat_fast(_ptr(np.ascontiguousarray(y)), y.shape[0], y.shape[1], _ptr(fs))
    assert np.array_equal(fs, R.fast_scores(y))
    cand = np.where(fs >= 20, np.clip(fs, 0, 255), 0).astype(np.uint8)
    cand[:1], cand[-1:], cand[:, :1], cand[:, -1:] = 0, 0, 0, 0
    keep = np.zeros_like(cand)
    feat_emul.feat_nms(_ptr(cand), *cand.shape, _ptr(keep))
    ys, xs = R.nms(cand)
    assert set(zip(*np.nonzero(keep))) == set(zip(ys.tolist(), xs.tolist()))


def test_host_harness_equals_restatement_per_keypoint(feat_emul):
    rng = np.random.default_rng(3)
    sm = rng.integers(0, 256, (120, 140), dtype=np.uint8)
    sm[30:90, 20:70] = rng.integers(0, 60, (60, 50))
    xs, ys = rng.integers(16, 140 - 16, 300), rng.integers(16, 120 - 16, 300)
    xy = np.stack([xs, ys], 1).astype(np.int32)
    bv = R.bin_vectors().astype(np.int32)
    out = np.zeros((300, 3), np.int32)
    feat_emul.feat_orient(_ptr(sm), sm.shape[1], _ptr(xy), 300, _ptr(bv), _ptr(out))
    m10, m01 = R.moments(sm, xs, ys)
    assert np.array_equal(out[:, 0], m10) and np.array_equal(out[:, 1], m01)
    assert np.array_equal(out[:, 2], R.orient_bins(m10, m01))
    a = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    b[100], b[250], b[17] = a[4], a[4], a[9] ^ 3
    d1, idx, d2 = R.best(R.distances(a, b))
    for chunk in (256, 64, 7):
        got = np.zeros((200, 3), np.int32)
        feat_emul.feat_best(_ptr(a), 200, _ptr(b), 300, chunk, _ptr(got))
        assert np.array_equal(got, np.stack([d1, idx, d2], 1)), chunk


# ---- the library without a device ---------------------------------------------------------------------------------------------------
def test_product_pattern_and_bin_vectors_equal_restatement(product_lib):
    out = np.zeros((30, 256, 4), np.int8)
    assert product_lib.v1c_feat_pattern(_ptr(out)) == 0
    assert np.array_equal(out, R.pattern())
    assert product_lib.v1c_feat_pattern(None) == -1


def test_feat_argument_validation_without_device(product_lib):
    from vr180_convert_amd import features as F

    buf = np.zeros(1 << 16, np.uint8)  # stands in for device pointers: validation fails before any device call
    kp, cnt = np.zeros(8192 * 6, np.int32), np.zeros(1, np.int32)

    def det(h=512, w=512, cn=3, p=None, img=_ptr(buf)):
        p = p or F.params(1.0, 256.0)
        return product_lib.v1c_feat_detect(0, None, img, h, w, w * cn, cn, C.byref(p), _ptr(kp), _ptr(buf), _ptr(cnt))

    def err():
        return product_lib.v1c_last_error().decode()

    assert det(cn=2) == -1 and "cn" in err()
    assert det(img=None) == -1 and "NULL" in err()
    assert det(p=F.params(0.0, 256.0)) == -1 and "scale" in err()
    assert det(p=F.params(1.5, 256.0)) == -1 and "scale" in err()
    assert det(p=F.params(0.05, 256.0)) == -1 and "smaller than the pattern" in err()
    assert det(p=F.params(1.0, 10.0)) == -1 and "empty circle" in err()
    assert det(p=F.params(1.0, 256.0, per_cell=9)) == -1 and "out of range" in err()
    p = F.params()
    assert product_lib.v1c_feat_match(0, None, None, 4, _ptr(buf), 4, C.byref(p), _ptr(kp), _ptr(kp), _ptr(cnt)) == -1
    assert product_lib.v1c_feat_match(0, None, _ptr(buf), -1, _ptr(buf), 4, C.byref(p), _ptr(kp), _ptr(kp), _ptr(cnt)) == -1
    assert product_lib.v1c_feat_match(0, None, _ptr(buf), 4, _ptr(buf), 4, C.byref(F.params(max_distance=300)), _ptr(kp), _ptr(kp),
                                      _ptr(cnt)) == -1


def test_feat_python_type_checks():
    from vr180_convert_amd import features as F

    with pytest.raises(TypeError):
        F._image_tensor(np.zeros((64, 64, 3), np.uint16), None)
    with pytest.raises(TypeError):
        F._image_tensor(np.zeros((64, 64, 3), np.float32), None)
    with pytest.raises(TypeError):
        F.params(bogus=1)


def test_kernels_feat_use_no_scratch_and_spill_nothing(tmp_path, product_lib):
    llvm = Path("/opt/rocm/lib/llvm/bin")
    obj = ROOT / "vr180_convert_amd" / "csrc" / "kernels_feat.o"
    assert obj.exists(), "kernels_feat.o is built by __graft_entry__.build() / make"
    shutil.copy(obj, tmp_path / "o.o")
    subprocess.run([str(llvm / "llvm-objdump"), "--offloading", "o.o"], cwd=tmp_path, check=True, capture_output=True, timeout=300)
    code = [p for p in tmp_path.iterdir() if "gfx950" in p.name]
    assert len(code) == 1
    text = subprocess.run([str(llvm / "llvm-readelf"), "--notes", code[0].name], cwd=tmp_path, check=True, capture_output=True,
                          text=True, timeout=300).stdout
    import yaml

    doc = text[text.index("---"):]
    doc = doc[: doc.index("\n...")] if "\n..." in doc else doc
    kernels = yaml.safe_load(doc)["amdhsa.kernels"]
    assert len(kernels) >= 9 and all("k_feat_" in k[".name"] for k in kernels)
    bad = [(k[".name"], k[".private_segment_fixed_size"], k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for k in kernels
           if k[".private_segment_fixed_size"] or k[".sgpr_spill_count"] or k[".vgpr_spill_count"]]
    assert not bad, bad
    assert all(k[".wavefront_size"] == 64 for k in kernels)


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------
def test_devfm_cli_glue(tmp_path, monkeypatch):
    """`devfm0.5` hands scale 0.5 and the radius to match_points_device, fits through rotation_match_robust and gives each eye its half
    rotator; --savematch keeps its warning (nothing is drawn without cv2)."""
    from typer.testing import CliRunner

    from vr180_convert_amd import _io, calibration, cli, features, quat, remapper
    from vr180_convert_amd.synth import pattern

    seen = {}
    rng = np.random.default_rng(0)
    pts = rng.uniform(20, 100, (40, 2))

    def fake_match(im1, im2, *, scale=1, radius="auto"):
        seen["match"] = (im1.shape, scale, radius)
        return pts, pts + 0.5, None, None, None, im1, im2

    robust = calibration.rotation_match_robust

    def fake_robust(a, b, *k, **kw):
        seen["robust"] = len(a)
        return robust(a, b, *k, **kw)

    monkeypatch.setattr(features, "match_points_device", fake_match)
    monkeypatch.setattr(cli, "rotation_match_robust", fake_robust)
    monkeypatch.setattr(remapper, "apply_lr", lambda *a, **k: seen.setdefault("apply_lr", a[0]))
    warnings = []
    monkeypatch.setattr(cli.LOG, "warning", lambda msg, *a, **k: warnings.append(str(msg)))
    l, r = tmp_path / "L.png", tmp_path / "R.png"
    _io.imwrite(l, pattern(128, 128)), _io.imwrite(r, pattern(128, 128))
    res = CliRunner().invoke(cli.app, ["lr", str(l), str(r), "--radius", "max", "--size", "64x64", "--automatch", "devfm0.5", "--savematch",
                                       "--out-path", str(tmp_path / "o.png")])
    assert res.exit_code == 0, (res.stdout, res.exception)
    assert seen["match"] == ((128, 128, 3), 0.5, "max") and seen["robust"] == 40
    assert any("--savematch ignored" in m for m in warnings) and not (tmp_path / "o.match.png").exists()
    # the chain each eye got: head * Euclidean3DRotator(half) * tail with calibration_rotators of the robust fit
    vl, vr = calibration.match_lr(cli.split_at_first_encoder(cli.parse_transformer(""))[1], pts, pts + 0.5, in_paths=[l, r], radius="max")
    q, _ = robust(vl, vr)
    ql, qr = calibration.calibration_rotators(q)
    left, right = seen["apply_lr"]
    rots = [next(s for s in t.transformers if type(s).__name__ == "Euclidean3DRotator") for t in (left, right)]
    assert np.allclose(quat.as_rotation_matrix(rots[0].rotation), quat.as_rotation_matrix(ql))
    assert np.allclose(quat.as_rotation_matrix(rots[1].rotation), quat.as_rotation_matrix(qr))
    res = CliRunner().invoke(cli.app, ["lr", str(l), str(r), "--radius", "max", "--size", "64x64", "--automatch", "devfm"])
    assert res.exit_code == 0 and seen["match"][1] == 1


def test_keypoints_keep_off_every_image_edge_whatever_the_radius_and_margin():
    """No qualifying row or column within BORDER of an edge: a landscape frame with a radius above h / 2, and margins below 16."""
    from vr180_convert_amd.synth import noise_disc

    rg = R.disc_ranges(1080, 1920, 1.0, 960.0, 19)
    assert (rg[:R.BORDER, 0] > rg[:R.BORDER, 1]).all() and (rg[-R.BORDER:, 0] > rg[-R.BORDER:, 1]).all()
    assert (rg[R.BORDER:-R.BORDER, 0] <= rg[R.BORDER:-R.BORDER, 1]).all()
    rng = np.random.default_rng(11)
    cases = [(rng.integers(0, 256, (270, 480, 3), dtype=np.uint8), 240.0, 19, 1.0),
             (rng.integers(0, 256, (540, 960, 3), dtype=np.uint8), 480.0, 19, 0.5),
             (noise_disc(256, 256, 3), 128.0, 0, 1.0), (noise_disc(256, 256, 3), 128.0, 8, 1.0)]
    for img, radius, margin, s in cases:
        kp, desc = R.detect(img, radius=radius, scale=s, margin=margin)
        ww, wh = R.working_size(img.shape[0], img.shape[1], s)
        assert len(kp) > 50 and desc.shape == (len(kp), 32)
        assert kp[:, 0].min() >= R.BORDER and kp[:, 0].max() <= ww - 1 - R.BORDER
        assert kp[:, 1].min() >= R.BORDER and kp[:, 1].max() <= wh - 1 - R.BORDER


def test_devfm_scale_outside_the_unit_interval_is_a_usage_error(tmp_path):
    from typer.testing import CliRunner

    from vr180_convert_amd import _io, cli
    from vr180_convert_amd.synth import pattern

    img = tmp_path / "a.png"
    _io.imwrite(img, pattern(64, 64))
    for opt in ("devfm2", "devfm0", "devfm1.5"):
        r = CliRunner().invoke(cli.app, ["lr", str(img), str(img), "--radius", "max", "--size", "32x32", "--automatch", opt])
        assert r.exit_code == 2 and "(0, 1]" in r.output, (opt, r.output, r.exception)
