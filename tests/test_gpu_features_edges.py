"""Feature matching (--automatch devfm) on the MI355X away from its defaults, bit-exact against the NumPy restatement (feat_ref.py): the
matcher with several LDS tiles per chunk and ties on the tile and chunk edges, selection with cells of 8 ... 64 pixels and caps of 1 ... N,
a cap that falls inside a class of equal scores, detects that find nothing, pitched / offset / strided views, the smallest working sizes,
and radius="auto" -- the default, negative on an image circle on black -- through detect, match_points_device and the CLI."""
import numpy as np
import pytest
import torch

import feat_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    from vr180_convert_amd import _native, features

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    _native.lib()
    return features


def _equal(got, want):
    return len(got) == len(want) and all(np.shape(g) == np.shape(w) and np.array_equal(g, w) for g, w in zip(got, want))


def _same_detect(F, img, ref_img=None, **kw):
    """device detect of `img` (an array or a device view) == the restatement on `ref_img` (the materialised array), shapes included"""
    ref_img = img if ref_img is None else ref_img
    got, want = F.detect(img, **kw), R.detect(ref_img, **kw)
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (got[0].shape, want[0].shape)
    assert got[0].dtype == np.int32 and got[1].dtype == np.uint8
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return got


# ---- 1. the matcher with several tiles per chunk ------------------------------------------------------------------------------------
# match_plan (kernels_feat.hip) as it stands, for nq queries against nt candidates, tiles of 256:
#     qblocks = ceil(nq / 256);  n = min(ceil(nt / 256), max(1, ceil(2048 / qblocks)), 64)
#     chunk = ceil(ceil(nt / n) / 256) * 256;  nch = ceil(nt / chunk)
#   nq   300, nt 17000: qblocks  2, n = min(67, 1024, 64) = 64, per 266 -> chunk 512, 34 chunks, the last one of 104 candidates
#   nq 17000, nt  9000: qblocks 67, n = min(36,   31, 64) = 31, per 291 -> chunk 512, 18 chunks, the last one of 296 (a tile + 40)
#   nq  9000, nt 17000: qblocks 36, n = min(67,   57, 64) = 57, per 299 -> chunk 512, 34 chunks
#   nq     1, nt 40000: qblocks  1, n = min(157, 2048, 64) = 64, per 625 -> chunk 768, 53 chunks, the last one of 64
#   (the other directions -- nt 300, nt 1 -- are single tiles.)  So every case below runs the tile loop two or three times per chunk, a
#   partial last tile inside a multi-tile chunk, and k_feat_merge over 18 ... 53 partial results.  _plan restates the arithmetic: if
#   match_plan changes, rework the table and the planted indices (tile edge 255 | 256, chunk edges 511 | 512 and 767 | 768).
def _plan(nq, nt):
    qblocks = -(-nq // 256)
    n = min(-(-nt // 256), max(1, -(-2048 // qblocks)), 64)
    chunk = -(-(-(-nt // n)) // 256) * 256
    return chunk, -(-nt // chunk)


def test_the_matcher_cases_have_several_tiles_per_chunk():
    assert _plan(300, 17000) == (512, 34) and _plan(17000, 9000) == (512, 18) and _plan(9000, 17000) == (512, 34)
    assert _plan(1, 40000) == (768, 53) and _plan(17000, 300) == (256, 2) and _plan(40000, 1) == (256, 1)
    assert _plan(4096, 4096) == (256, 16)  # the largest set of test_gpu_features.py: one tile per chunk


ZERO_TIE = (255, 256, 511, 512, -1)  # candidates equal to one query: the tile edge, the chunk edge of 512, the last index
NEAR_TIE = (767, 768, 1023, 1024)    # candidates one bit off another query: tile / chunk edges again (768: the chunk edge of 1 x 40000)


def _sets(nq, nt, ties):
    """random descriptors as in test_matcher_equals_brute_force (a third of the smaller set are near copies: matches), and for every
    entry of `ties` one query, from the last one backwards, with tied best candidates: "zero" -- ZERO_TIE hold the query itself -- or
    "near" -- NEAR_TIE hold it with one bit flipped.  Returns the sets and {kind: query}"""
    rng = np.random.default_rng(nq + nt)
    a = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    k = min(nq, nt) // 3
    a[:k] = b[rng.integers(0, nt, k)] ^ rng.integers(0, 2, (k, 32), dtype=np.uint8)
    where = {}
    for n, tie in enumerate(ties):
        q = where[tie] = nq - 1 - n
        if tie == "zero":
            b[list(ZERO_TIE)] = a[q]
        else:
            b[list(NEAR_TIE)] = a[q]
            b[list(NEAR_TIE), 7] ^= 16
    return a, b, where


LOOSE = {"max_distance": 256, "ratio": (1, 1)}


@pytest.mark.parametrize("na,nb,ties", [(300, 17000, ("zero", "near")), (17000, 9000, ("zero", "near")), (1, 40000, ("zero",)),
                                        (1, 40000, ("near",)), (40000, 1, ("zero",)), (40000, 1, ("near",))])
def test_matcher_with_several_tiles_per_chunk_and_ties_on_their_edges(F, na, nb, ties):
    small, large, where = _sets(min(na, nb), max(na, nb), ties)  # the ties lie among the candidates of the larger set
    rows, cols = R.best_both(small, large)  # one pass over the distances serves both argument orders and both parameter sets
    for tie, q in where.items():  # the restatement itself, first: the lower index wins, d2 == d1
        assert (rows[0][q], rows[1][q], rows[2][q]) == ((0, ZERO_TIE[0], 0) if tie == "zero" else (1, NEAR_TIE[0], 1)), tie
    orders = [(small, large, rows, cols), (large, small, cols, rows)]
    for x, y, rx, ry in orders if na <= nb else orders[::-1]:
        for kw in ({}, LOOSE):
            got = F.match(x, y, **kw)
            want = R.match_from_best(rx, ry, **kw)
            assert _equal(got, want), (len(x), len(y), kw, len(got[0]), len(want[0]))
            assert len(want[0]) >= min(na, nb) // 5 or min(na, nb) == 1  # (the planted near copies: plenty of matches)
            if x is not small:
                continue
            # a duplicate pair at distance 0 passes the ratio test (4 * 0 <= 3 * 0); a tied pair at distance 1 fails it (4 > 3) and
            # passes 1 / 1; either way the lower index wins
            kept = [tuple(int(v) for v in t) for t in zip(*got)]
            if "zero" in where:
                assert (where["zero"], ZERO_TIE[0], 0) in kept
            if "near" in where:
                assert ((where["near"], NEAR_TIE[0], 1) in kept) == (kw is LOOSE)
                assert kw is LOOSE or where["near"] not in [t[0] for t in kept]


# ---- 2. selection and cap -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def disc512():
    from vr180_convert_amd.synth import noise_disc

    return noise_disc(512, 512, 7)


@pytest.mark.parametrize("per_cell", [1, 3, 4])
@pytest.mark.parametrize("cell", [8, 47, 64])
def test_cells_of_8_47_and_64_pixels(F, disc512, cell, per_cell):
    """cell 8 and 64: the limits of the validation (k_feat_select: 1 and 16 keys per lane); 47 divides neither 512 nor the tile sizes"""
    kp, _ = _same_detect(F, disc512, radius=256.0, cell=cell, per_cell=per_cell, max_keypoints=65536)
    ncx = -(-512 // cell)
    cidx = (kp[:, 1] // cell) * ncx + kp[:, 0] // cell
    assert len(kp) > 40 and (np.diff(cidx) >= 0).all() and np.bincount(cidx).max() == per_cell  # cell-major, per_cell reached


def test_caps_of_1_2_n_and_n_minus_1(F, disc512):
    full, _ = R.detect(disc512, radius=256.0)
    n = len(full)
    assert 300 < n < 8192  # uncapped at the default cap
    for cap in (1, 2, n, n - 1):
        kp, _ = _same_detect(F, disc512, radius=256.0, max_keypoints=cap)
        assert len(kp) == cap


def tie_class_image():
    """one corner motif -- a bright 7 x 7 square on dark -- every 16 pixels of a 512 x 512 canvas: with cells of 16 pixels every cell holds
    the same pixels, so the keypoints fall into a few large classes of equal score"""
    tile = np.full((16, 16), 30, np.uint8)
    tile[4:11, 4:11] = 220
    return np.ascontiguousarray(np.repeat(np.tile(tile, (32, 32))[..., None], 3, axis=2))


TIE_KW = {"radius": 256.0, "cell": 16, "per_cell": 2, "fast_threshold": 20}


def test_a_cap_inside_a_class_of_equal_scores_keeps_the_first_in_cell_rank_order(F):
    img = tie_class_image()
    full, _ = R.detect(img, max_keypoints=65536, **TIE_KW)
    scores = full[:, 2]
    assert len(np.unique(scores)) == 1 and len(full) > 300, (np.unique(scores, return_counts=True), len(full))
    capped, _ = R.detect(img, max_keypoints=100, **TIE_KW)
    assert np.array_equal(capped, full[:100])  # one class, and `full` is in (cell, rank) order
    kp, _ = _same_detect(F, img, max_keypoints=100, **TIE_KW)
    assert np.array_equal(kp[:, :3], full[:100, :3])


# ---- 3. nothing found ---------------------------------------------------------------------------------------------------------------
def test_no_keypoint_and_empty_sets(F):
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 256, (200, 300, 3), dtype=np.uint8)
    for img, kw in ((np.full((200, 300, 3), 128, np.uint8), {}), (noise, {"fast_threshold": 255})):
        kp, desc = _same_detect(F, img, radius=100.0, **kw)
        assert kp.shape == (0, 6) and desc.shape == (0, 32)
    d = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    for x, y in ((desc, d), (d, desc), (desc, desc)):
        got = F.match(x, y)
        assert len(got) == 3 and all(g.shape == (0,) for g in got)
        assert all(len(w) == 0 for w in R.match_blocked(x, y))


# ---- 4. views -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_the_halves_of_a_side_by_side_tensor(F, cn):
    """pitched views (stride(0) == 2 * w * cn), the right one at a byte offset of w * cn (odd for 211 x 1 and 211 x 3)"""
    rng = np.random.default_rng(40 + cn)
    h, w = 190, 211
    sbs = rng.integers(0, 256, (h, 2 * w, cn), dtype=np.uint8)
    dev = torch.from_numpy(sbs).cuda()
    for t, ref in ((dev[:, :w], sbs[:, :w]), (dev[:, w:], sbs[:, w:])):
        assert not t.is_contiguous()
        kp, _ = _same_detect(F, t, np.ascontiguousarray(ref), radius=100.0, scale=1.0)
        assert len(kp) > 30
    if cn == 3:  # ... and through match_points_device, against contiguous copies: the same bytes
        right = np.roll(sbs[:, :w], (2, 3), axis=(0, 1))
        dev[:, w:] = torch.from_numpy(right).cuda()
        a = F.match_points_device(dev[:, :w], dev[:, w:], radius=100.0)
        b = F.match_points_device(dev[:, :w].contiguous(), torch.from_numpy(right).cuda(), radius=100.0)
        assert len(a[0]) > 20
        for x, y in zip(a[:5], b[:5]):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_offset_row_sliced_and_column_strided_views(F):
    rng = np.random.default_rng(44)
    h, w, cn = 240, 283, 3
    img = rng.integers(0, 256, (h, w, cn), dtype=np.uint8)
    flat = torch.from_numpy(np.concatenate([rng.integers(0, 256, 1, dtype=np.uint8), img.reshape(-1)])).cuda()
    odd = flat[1:].view(h, w, cn)
    assert odd.data_ptr() % 2 == 1 and odd.is_contiguous()
    dev = torch.from_numpy(img).cuda()
    views = {"odd byte offset": odd, "rows 5 ... h - 9": dev[5:h - 9], "every second row": dev[::2], "every second column": dev[:, ::2],
             "rows and columns": dev[3::2, 1:w - 7]}
    for name, t in views.items():
        kp, _ = _same_detect(F, t, np.ascontiguousarray(t.cpu().numpy()), radius=1e4, margin=0)
        assert len(kp) > 20, name
    assert not views["every second row"].is_contiguous() and views["every second column"].stride(1) == 2 * cn


# ---- 5. the smallest and the tile-edge working sizes --------------------------------------------------------------------------------
def _source_size(n_work, s):
    n = int(n_work / s) - 2
    while int(n * s) < n_work:
        n += 1
    assert int(n * s) == n_work
    return n


@pytest.mark.parametrize("scale", [1.0, 1 / 3, 0.37])
@pytest.mark.parametrize("wh,ww", [(33, 33), (33, 65), (48, 128), (49, 129), (63, 64)])
def test_smallest_and_tile_edge_working_sizes(F, wh, ww, scale):
    """33 x 33: the smallest the pattern allows, where only working pixel (16, 16) can qualify; 64 / 65, 128 / 129: the 64-lane rows of
    the pixel kernels and the smoothing tile (64 x 16); 48 / 49, 63: rows against the tile and the 4-row blocks.  The source block of
    working pixel (16, 16) is white on noise of 0 ... 99, so that there is a corner to find."""
    h, w = _source_size(wh, scale), _source_size(ww, scale)
    assert R.working_size(h, w, scale) == (ww, wh)
    rng = np.random.default_rng(wh * 1000 + ww)
    img = rng.integers(0, 100, (h, w, 3), dtype=np.uint8)
    rb, cb = R.bounds(wh, h, scale), R.bounds(ww, w, scale)
    img[rb[16]:rb[17], cb[16]:cb[17]] = 255
    kp, _ = _same_detect(F, img, radius=1e4, scale=scale, margin=0, fast_threshold=5)
    assert (16, 16) in [(int(x), int(y)) for x, y in kp[:, :2]]
    if (wh, ww) == (33, 33):
        assert len(kp) == 1


def test_a_working_size_of_32_is_refused(F):
    for h, w, s in ((32, 40, 1.0), (40, 32, 1.0), (_source_size(33, 1 / 3) - 1, 120, 1 / 3)):
        assert min(R.working_size(h, w, s)) == 32 and R.refusal(h, w, s, 1e4, 0) == "working image under 33 x 33"
        with pytest.raises(ValueError, match="smaller than the pattern needs"):
            F.detect(np.zeros((h, w, 3), np.uint8), radius=1e4, scale=s, margin=0)


# ---- 6. radius="auto", the default --------------------------------------------------------------------------------------------------
def textured_disc(h, w, r, seed):
    """noise_disc-like, but with black around the circle: noise of 30 ... 255 within r of the centre, so that get_radius finds both edges"""
    rng = np.random.default_rng(seed)
    img = rng.integers(30, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:h, :w]
    img[(xx - w // 2) ** 2 + (yy - h // 2) ** 2 > r * r] = 0
    return img


def auto_pair(h, w, r, seed):
    """a disc and the same disc moved by (2, 3) pixels under a little noise: hundreds of matches"""
    left = textured_disc(h, w, r, seed)
    rng = np.random.default_rng(seed + 1)
    right = np.roll(left, (2, 3), axis=(0, 1)).astype(np.int16)
    right = np.where(right > 0, np.clip(right + rng.integers(-2, 3, right.shape), 30, 255), 0).astype(np.uint8)
    return left, right


@pytest.mark.parametrize("h,w,r", [(480, 640, 200), (512, 512, 230)])
def test_auto_radius_of_an_image_circle_on_black(F, h, w, r):
    """radius="auto" is the default of match_points_device and of `lr --radius`; on an image circle on black the reference's get_radius
    is negative, which v1c_feat_detect refuses ("radius must lie in (0, 1e9]"): features.resolve_radius hands over the magnitude"""
    from vr180_convert_amd.chain import get_radius
    from vr180_convert_amd.remapper import get_radius_smart

    left, right = auto_pair(h, w, r, h + r)
    assert get_radius(left) == -(r + 0.5) and get_radius(right) < 0
    shared = get_radius_smart("auto", [left, right])
    assert shared < 0
    for img in (left, torch.from_numpy(right).cuda()):
        one = get_radius_smart("auto", [img])
        got, want = F.detect(img, radius="auto"), F.detect(img, radius=abs(one))
        assert one < 0 and len(got[0]) > 150 and all(g.tobytes() == w_.tobytes() for g, w_ in zip(got, want))
    _same_detect(F, left, radius=r + 0.5)
    got = F.match_points_device(left, right)
    want = F.match_points_device(left, right, radius=abs(shared))
    assert len(got[0]) > 100
    for x, y in zip(got[:5], want[:5]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_cli_devfm_with_the_default_radius(F, tmp_path):
    from typer.testing import CliRunner

    from vr180_convert_amd import _io, cli
    from vr180_convert_amd import transformer as T
    from vr180_convert_amd.calibration import calibration_rotators, match_lr, rotation_match_robust
    from vr180_convert_amd.remapper import apply_lr

    l, r = tmp_path / "L.png", tmp_path / "R.png"
    left, right = auto_pair(512, 512, 230, 9)
    _io.imwrite(l, left), _io.imwrite(r, right)
    out = tmp_path / "out.png"
    res = CliRunner().invoke(cli.app, ["lr", str(l), str(r), "--automatch", "devfm", "--size", "256x256", "--out-path", str(out)])
    assert res.exit_code == 0, (res.stdout, res.exception)
    il, ir = _io.imread(l), _io.imread(r)
    head, tail = cli.split_at_first_encoder(cli.parse_transformer(""))
    p1, p2 = F.match_points_device(il, ir)[:2]
    q, _ = rotation_match_robust(*match_lr(tail, p1, p2, in_paths=[l, r], radius="auto"))
    ql, qr = calibration_rotators(q)
    want = tmp_path / "want.png"
    apply_lr((head * T.Euclidean3DRotator(ql) * tail, head * T.Euclidean3DRotator(qr) * tail), left_path=l, right_path=r, out_path=want,
             radius="auto", size_output=(256, 256))
    assert np.array_equal(_io.imread(out), _io.imread(want))


def test_auto_radius_without_a_black_border_keeps_raising_index_error(F):
    noise = np.random.default_rng(5).integers(30, 256, (200, 200, 3), dtype=np.uint8)
    with pytest.raises(IndexError):
        F.detect(noise, radius="auto")
    with pytest.raises(IndexError):
        F.match_points_device(torch.from_numpy(noise).cuda(), noise)
