"""Feature matching (--automatch devfm) on the MI355X: keypoints, descriptors and matches bit-exact against the NumPy restatement
(feat_ref.py), the matcher against brute force, rotation recovery on rendered sphere scenes (sphere_scene.py), the CLI end to end without
cv2, errors and determinism."""
from pathlib import Path

import numpy as np
import pytest
import torch

import feat_ref as R
import sphere_scene as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def F():
    from vr180_convert_amd import _native, features

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    _native.lib()
    return features


@pytest.fixture(scope="module")
def pair768():
    return S.render(768), S.render(768, S.rotation([0.3, 1, 0.2], 4))


@pytest.fixture(scope="module")
def left2048():
    return S.render(2048)


def _same_detect(F, img, radius, scale, **kw):
    kp, desc = F.detect(img, radius=radius, scale=scale, **kw)
    kp_r, desc_r = R.detect(img, radius=radius, scale=scale, **kw)
    assert len(kp) > 0 and kp.shape == kp_r.shape, (kp.shape, kp_r.shape)
    assert np.array_equal(kp, kp_r)
    assert np.array_equal(desc, desc_r)
    return kp, desc


# ---- 1. bit-exact against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_noise_disc_bit_exact(F, cn):
    from vr180_convert_amd.synth import noise_disc

    img = noise_disc(512, 512, 2, cn=cn)
    _same_detect(F, img if cn > 1 else img[..., 0], 256.0, 1.0)


@pytest.mark.parametrize("scale", [1.0, 0.5, 0.37])
def test_sphere_pair_bit_exact(F, pair768, scale):
    (kl, dl), (kr, dr) = (_same_detect(F, im, 384.0, scale) for im in pair768)
    got = F.match(dl, dr)
    want = R.match(dl, dr)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and len(got[0]) > 20


def test_reference_photo_bit_exact(F):
    from vr180_convert_amd import _io

    img = _io.imread(ROOT / "tests" / "golden" / "ref_docs" / "test.jpg")
    _same_detect(F, img, img.shape[0] / 2, 0.25)


def test_cap_keeps_the_first_n_max_in_score_cell_rank_order(F):
    from vr180_convert_amd.synth import noise_disc

    img = noise_disc(512, 512, 5)
    full, _ = R.detect(img, radius=256.0, per_cell=4, cell=16)
    assert len(full) > 1000
    kp, _ = _same_detect(F, img, 256.0, 1.0, per_cell=4, cell=16, max_keypoints=777)
    assert len(kp) == 777 and kp[:, 2].min() >= np.sort(full[:, 2])[::-1][776]


# ---- 2. matcher against brute force -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("na,nb", [(4096, 4096), (1, 700), (700, 1), (3000, 257)])
def test_matcher_equals_brute_force(F, na, nb):
    rng = np.random.default_rng(na + nb)
    a = rng.integers(0, 256, (na, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    k = min(na, nb) // 3
    a[:k] = b[rng.integers(0, nb, k)] ^ rng.integers(0, 2, (k, 32), dtype=np.uint8)  # near copies: matches
    if nb > 10:
        b[5] = b[7] = a[0]  # a tie for a[0]
    for x, y in ((a, b), (b, a)):
        for kw in ({}, {"max_distance": 256, "ratio": (1, 1)}):
            got = F.match(x, y, **kw)
            want = R.match(x, y, **kw)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (na, nb, kw)


# ---- 3. rotation recovery -----------------------------------------------------------------------------------------------------------
CASES = {"identity": ([0, 0, 1], 0.0), "yaw1": ([0, 1, 0], 1.0), "pitch3_yaw2": (None, None), "roll8": ([0, 0, 1], 8.0),
         "axis5": ([0.42, -0.71, 0.57], 5.0)}


def _rot(name):
    axis, deg = CASES[name]
    if axis is None:
        return S.rotation([1, 0, 0], 3) @ S.rotation([0, 1, 0], 2)
    return S.rotation(axis, deg)


def _angle_deg(q1, q2):
    a = np.array([q1.w, q1.x, q1.y, q1.z]) / np.linalg.norm([q1.w, q1.x, q1.y, q1.z])
    b = np.array([q2.w, q2.x, q2.y, q2.z]) / np.linalg.norm([q2.w, q2.x, q2.y, q2.z])
    return np.degrees(2 * np.arccos(min(1.0, abs(float(a @ b)))))


def _recover(F, left, right, rot, scale):
    from vr180_convert_amd import cli
    from vr180_convert_amd.calibration import match_lr, rotation_match, rotation_match_robust

    n = left.shape[0]
    tail = cli.split_at_first_encoder(cli.parse_transformer(""))[1]
    p1, p2, kp1, kp2, matches, _, _ = F.match_points_device(left, right, scale=scale, radius="max")
    assert len(p1) >= 200, len(p1)
    # no kept match near the rim: every keypoint lies within r * s - margin of the centre (working pixels)
    for kp in (kp1[matches[:, 0]], kp2[matches[:, 1]]):
        c = (n // 2) * scale
        assert (np.hypot(kp[:, 0] - c, kp[:, 1] - c) <= n / 2 * scale - 19).all()
    q, _ = rotation_match_robust(*match_lr(tail, p1, p2, in_paths=[left, right], radius="max"))
    w = S.directions(500, 70)
    t1, t2 = S.project(n, w), S.project(n, w @ rot)  # rot^T w, row-wise
    q_true = rotation_match(*match_lr(tail, t1, t2, in_paths=[left, right], radius="max"))
    return _angle_deg(q, q_true), len(p1)


@pytest.mark.parametrize("name", list(CASES))
def test_rotation_recovery_2048(F, left2048, name):
    right = S.render(2048, _rot(name))
    errs = {}
    for scale, limit in ((1.0, 0.05), (0.5, 0.1)):
        err, n = _recover(F, left2048, right, _rot(name), scale)
        errs[scale] = (round(err, 4), n)
        assert err <= limit, (name, errs)
    print(name, errs)


def test_rotation_recovery_4096(F):
    rot = _rot("pitch3_yaw2")
    left, right = S.render(4096), S.render(4096, rot)
    for scale, limit in ((1.0, 0.05), (0.5, 0.1)):
        err, n = _recover(F, left, right, rot, scale)
        assert err <= limit, (scale, err, n)


# ---- 4. the CLI without cv2 ---------------------------------------------------------------------------------------------------------
def test_cli_devfm_end_to_end_without_cv2(F, tmp_path, monkeypatch):
    import builtins
    import sys

    from typer.testing import CliRunner

    from vr180_convert_amd import _io, cli
    from vr180_convert_amd import transformer as T
    from vr180_convert_amd.calibration import calibration_rotators, match_lr, rotation_match_robust
    from vr180_convert_amd.remapper import apply_lr

    real_import = builtins.__import__
    monkeypatch.setattr(builtins, "__import__", lambda name, *a, **k: (_ for _ in ()).throw(ImportError("no cv2")) if name == "cv2" else real_import(name, *a, **k))
    monkeypatch.delitem(sys.modules, "cv2", raising=False)
    monkeypatch.setattr(_io, "_cv", None)
    l, r = tmp_path / "L.png", tmp_path / "R.png"
    _io.imwrite(l, S.render(1024)), _io.imwrite(r, S.render(1024, _rot("pitch3_yaw2")))
    out = tmp_path / "out.png"
    res = CliRunner().invoke(cli.app, ["lr", str(l), str(r), "--automatch", "devfm", "--radius", "max", "--size", "256x256",
                                       "--out-path", str(out)])
    assert res.exit_code == 0, (res.stdout, res.exception)
    il, ir = _io.imread(l), _io.imread(r)
    head, tail = cli.split_at_first_encoder(cli.parse_transformer(""))
    p1, p2 = F.match_points_device(il, ir, radius="max")[:2]
    q, _ = rotation_match_robust(*match_lr(tail, p1, p2, in_paths=[l, r], radius="max"))
    ql, qr = calibration_rotators(q)
    want = tmp_path / "want.png"
    apply_lr((head * T.Euclidean3DRotator(ql) * tail, head * T.Euclidean3DRotator(qr) * tail), left_path=l, right_path=r, out_path=want,
             radius="max", size_output=(256, 256))
    assert np.array_equal(_io.imread(out), _io.imread(want))


# ---- 5. errors, 6. determinism ------------------------------------------------------------------------------------------------------
def test_black_pair_and_wide_types_raise(F):
    black = np.zeros((512, 512, 3), np.uint8)
    with pytest.raises(ValueError, match="0 match"):
        F.match_points_device(black, black, radius="max")
    with pytest.raises(TypeError):
        F.match_points_device(black.astype(np.uint16), black.astype(np.uint16), radius="max")
    with pytest.raises(TypeError):
        F.detect(torch.zeros((512, 512, 3), dtype=torch.float32, device="cuda"), radius=256.0)


def test_two_runs_give_identical_bytes(F, pair768):
    a = F.match_points_device(*pair768, radius="max")
    b = F.match_points_device(*(torch.from_numpy(im).cuda() for im in pair768), radius="max")
    for x, y in zip(a[:5], b[:5]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


@pytest.mark.parametrize("case", ["landscape_radius_above_half_height", "landscape_s0.5", "square_margin0", "square_margin8"])
def test_keypoints_near_the_image_edges_bit_exact(F, case):
    """Radii above h / 2 and margins below 16 reach the image edges: no keypoint may lie within 16 working pixels of any edge, and the
    device output still equals the restatement."""
    from vr180_convert_amd.synth import noise_disc

    rng = np.random.default_rng(11)
    img, radius, margin, s = {
        "landscape_radius_above_half_height": (rng.integers(0, 256, (270, 480, 3), dtype=np.uint8), 240.0, 19, 1.0),
        "landscape_s0.5": (rng.integers(0, 256, (540, 960, 3), dtype=np.uint8), 480.0, 19, 0.5),
        "square_margin0": (noise_disc(256, 256, 3), 128.0, 0, 1.0),
        "square_margin8": (noise_disc(256, 256, 3), 128.0, 8, 1.0)}[case]
    kp, _ = _same_detect(F, img, radius, s, margin=margin)
    ww, wh = R.working_size(img.shape[0], img.shape[1], s)
    assert kp[:, 0].min() >= R.BORDER and kp[:, 0].max() <= ww - 1 - R.BORDER
    assert kp[:, 1].min() >= R.BORDER and kp[:, 1].max() <= wh - 1 - R.BORDER
