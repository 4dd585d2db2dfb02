"""The launch record of the pair mirror kernels (csrc/tile_device.hpp: MirrorRec) without a GPU.

plan.hip turns every (tile box, band box) pair into one 64-byte record, once per plan; k_ray_lin3_pair_mirror_seq and the one-eye
k_ray_lin3_pair_mirror_raw read it instead of deriving the same numbers in every wave of every launch.  These tests hold the record
to the arithmetic it replaces, through the product's own __host__ __device__ functions compiled for the host (tests/host_mirror_rec):

* round trip: every decoded field equals the expression the kernels evaluated from the TileBox pair (units per row, rows per pass,
  lanes with a unit, first row of the last pass, passes of waves 0-3 and their first rows, pitches, mirror_raw_fit as a bit), for
  the tile pairs of C2's geometry, the mirror geometries of tests/test_gpu_parity.py and a sweep over every cpr and row count;
* lanes: the record's 16-bit magic yields lane / upr for every upr in 1..48 (and up to 64) and every lane -- the exact quotient and
  what raw_lanes_upr's fp32 reciprocal form yields, the reciprocal taken one unit in the last place either way too;
* the rounding trick: the coordinates stay biased by the bits of 1.5 * 2^23; the fractions and the tap addresses come out the same.

The boxes come from a host model of k_tile_boxes (the oracle's float32 map, cv2's 1/32 buckets, 64 x 16 tiles): the plan's boxes
proper are computed on the GPU (tests/test_gpu_mirror_record.py runs those)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import chainspecs as CS

ROOT = Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "host_mirror_rec" / "rec.hip"
BIAS = 0x4B400000
POLY = [("equirect_enc", True), ("poly", [0, 1, -0.1]), CS.EQUI]
EQUI = [("equirect_enc", True), CS.EQUI]

# (name, chain, source (h, w), output (w, h), radius)
GEOMETRIES = [
    ("c2_4096", POLY, (4096, 4096), (4096, 4096), 2048.0),
    ("300_448", EQUI, (300, 300), (448, 448), 150.0),
    ("512x640_544x576", EQUI, (512, 640), (544, 576), 250.0),
    ("1000_1028x1024", POLY, (1000, 1000), (1028, 1024), 470.0),
    ("1000_1028x1056", POLY, (1000, 1000), (1028, 1056), 470.0),
    ("120_1024", POLY, (120, 120), (1024, 1024), 60.0),
    ("900x1200_640", EQUI, (900, 1200), (640, 640), 450.0),
    ("rest_free_1024", POLY, (1024, 1024), (1024, 1024), 512.0),  # the GPU test's REST = 0 case
]


@pytest.fixture(scope="module")
def rec_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_mirror_rec") / "libv1c_mirror_rec.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-fno-fast-math", "-o", str(out),
                    str(HARNESS)], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(out))
    vp, i32 = C.c_void_p, C.c_int
    lib.rec_encode.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    lib.rec_decode.argtypes = [vp, vp]
    lib.rec_present.argtypes = [vp, vp, i32, i32, i32, vp]
    lib.rec_lane_forms.argtypes = [i32, i32, vp]
    lib.rec_tap_sweep.argtypes = [i32, i32, i32]
    lib.rec_tap_sweep.restype = C.c_int64
    assert lib.rec_sizeof() == 64
    return lib


def model_boxes(xm, ym, src_hw, mirror_h=0):
    """k_tile_boxes for a bilinear plan, on the host: the bounding box of the 2 x 2 footprints of each 64 x 16 tile's pixels, (TY, TX, 8)
    ints laid out like TileBox.  `mirror_h`: the boxes of the mirrored bands (rows mirror_h - j).  The table slice (idx0, nidx) needs the
    plan's radial table: interior tiles get the stand-in (0, 1)."""
    H, W = xm.shape
    src_h, src_w = src_hw
    if mirror_h:
        rows = np.clip(mirror_h - np.arange(H), 0, H - 1)
        xm, ym = xm[rows], ym[rows]
    ok = np.isfinite(xm) & np.isfinite(ym) & (np.abs(xm) < 2.0 ** 25) & (np.abs(ym) < 2.0 ** 25)
    sx = np.rint(np.where(ok, xm, 0).astype(np.float32) * np.float32(32)).astype(np.int64)
    sy = np.rint(np.where(ok, ym, 0).astype(np.float32) * np.float32(32)).astype(np.int64)
    ix, iy = sx >> 5, sy >> 5
    inside = ok & (ix >= 0) & (ix < max(src_w - 2, 0)) & (iy >= 0) & (iy < max(src_h - 1, 0))
    TY, TX = (H + 15) // 16, (W + 63) // 64

    def tiles(a, fill):
        p = np.full((TY * 16, TX * 64), fill, a.dtype)
        p[:H, :W] = a
        return p.reshape(TY, 16, TX, 64).transpose(0, 2, 1, 3).reshape(TY, TX, 1024)

    big = 1 << 20
    tin = tiles(inside, False)
    xmn = tiles(np.where(inside, ix, big), big).min(-1)
    ymn = tiles(np.where(inside, iy, big), big).min(-1)
    xmx = tiles(np.where(inside, ix, -big), -big).max(-1)
    ymx = tiles(np.where(inside, iy, -big), -big).max(-1)
    any_in = tin.any(-1)
    b = np.zeros((TY, TX, 8), np.int32)
    x0 = xmn & ~3
    b[..., 0] = np.where(any_in, x0, 0)
    b[..., 1] = np.where(any_in, ymn, 0)
    b[..., 2] = np.where(any_in, (xmx + 2 - x0 + 3) >> 2, 0)
    b[..., 3] = np.where(any_in, ymx - ymn + 2, 0)
    interior = tin.all(-1)  # (padding counts as outside: a ragged last tile column is not interior)
    b[..., 5] = interior
    b[..., 6] = interior
    return b


def raw_passes(b, q, th, permille, max_kb):
    """tile_mirror_raw_passes (kernels_mirror.hip): the smallest buffer, in KB, that holds the boxes of `permille` of the tile pairs"""
    upr = lambda c: (3 * c + 3) >> 2
    need = []
    for ty in range(th + 1):
        for tx in range(b.shape[1]):
            cb, cq = int(b[ty, tx, 2]), int(q[ty, tx, 2])
            if cb <= 0 or cq <= 0 or cb > 64 or cq > 64:
                continue
            u = max(int(b[ty, tx, 3]) * upr(cb), int(q[ty, tx, 3]) * upr(cq))
            need.append(min((u + 63) // 64, 17))
    hist = np.bincount(np.array(need, np.int64), minlength=18)
    acc = 0
    for k in range(17):
        acc += hist[k]
        if acc * 1000 >= len(need) * permille:
            return min(max(k, 4), max_kb)
    return max_kb


@pytest.fixture(scope="module")
def plans(oracle_mod):
    out = {}
    for name, spec, src_hw, out_wh, radius in GEOMETRIES:
        xm, ym = oracle_mod.get_map(spec, radius=radius, size_input=src_hw, size_output=out_wh)
        b, q = model_boxes(xm, ym, src_hw), model_boxes(xm, ym, src_hw, mirror_h=out_wh[1])
        th = b.shape[0] // 2
        out[name] = (b, q, src_hw, raw_passes(b, q, th, 998, 11), raw_passes(b, q, th, 980, 12))
    return out


def check_pair(lib, b8, q8, seq_kb, one_kb, src_h, src_w):
    """one tile pair: encode, decode, compare with the kernels' own expressions; returns (fit at seq_kb, fit at one_kb, upr of b, of q)"""
    w = np.zeros(16, np.uint32)
    got = np.zeros(27, np.int64)
    lib.rec_encode(b8.ctypes.data, q8.ctypes.data, seq_kb, one_kb, src_h, src_w, w.ctypes.data)
    lib.rec_decode(w.ctypes.data, got.ctypes.data)
    fits = []
    for bit, kb in ((2, seq_kb), (4, one_kb)):
        want = np.zeros(27, np.int64)
        lib.rec_present(b8.ctypes.data, q8.ctypes.data, kb, src_h, src_w, want.ctypes.data)
        fit = want[26] == 1
        assert bool(got[26] & bit) == bool(fit), (b8, q8, kb, got[26], want[26])
        fits.append(bool(fit))
        if not fit:
            continue
        assert bool(got[26] & 1) == bool(b8[6] & 2)
        for k in (0, 12):
            for f in (0, 1, 2, 3, 4, 5, 6, 8, 10, 11):  # (7: magic, 9: tapk -- their own tests)
                assert got[k + f] == want[k + f], (b8, q8, kb, k, f, got[k:k + 12], want[k:k + 12])
            upr = int(want[k + 4])
            assert got[k + 7] == (65536 + upr - 1) // upr
        assert got[24] == want[24] and got[25] == want[25]
    return fits[0], fits[1], int(got[4]), int(got[16])


@pytest.mark.parametrize("name", [g[0] for g in GEOMETRIES])
def test_record_round_trip_on_plans(rec_lib, plans, name):
    b, q, (src_h, src_w), seq_kb, one_kb = plans[name]
    TY, TX = b.shape[:2]
    n_fit = n_diff = 0
    for ty in range(TY // 2 + 1):
        for tx in range(TX):
            b8, q8 = np.ascontiguousarray(b[ty, tx]), np.ascontiguousarray(q[ty, tx])
            fs, fo, ub, uq = check_pair(rec_lib, b8, q8, seq_kb, one_kb, src_h, src_w)
            n_fit += fs
            n_diff += fs and ub != uq
    print(name, "tile pairs that fit", n_fit, "of", (TY // 2 + 1) * TX, "with b.upr != q.upr", n_diff, "seq KB", seq_kb, "one-eye KB", one_kb)
    assert n_fit > 0
    if name in ("c2_4096", "1000_1028x1056"):  # geometries with tile pairs whose tile and band boxes differ in width (b.upr != q.upr)
        assert n_diff > 0
    if name in ("c2_4096", "rest_free_1024"):  # empty rest list: every pair of tile rows 0 .. TY / 2 fits the seq buffers
        assert n_fit == (TY // 2 + 1) * TX


def test_record_round_trip_sweep(rec_lib):
    """every cpr, row counts around every multiple of the rows per pass, boxes at the image's end, boxes that do not fit"""
    rng = np.random.default_rng(5)
    n = 0
    for cpr in range(0, 66):
        upr = (3 * cpr + 3) >> 2
        R = 64 // max(upr, 1)
        rows = sorted({1, 2, 3, R - 1, R, R + 1, 2 * R, 4 * R - 1, 4 * R, 4 * R + 1, 7 * R + 3, 8 * R, 15, 16, 21, 40, 200, 1100} - {0, -1})
        for nrows in rows:
            for _ in range(2):
                x0, y0 = int(rng.integers(0, 2000)) * 4, int(rng.integers(0, 3000))
                cq, nq = int(rng.integers(1, 65)), int(rng.integers(1, 30))
                b8 = np.array([x0, y0, cpr, nrows, 7, 5, int(rng.choice([1, 3])), 0], np.int32)
                q8 = np.array([max(x0 - 4, 0), y0 + 40, cq, nq, 8, 3, b8[6], 0], np.int32)
                for src_h, src_w in ((8192, 8192), (y0 + nrows, x0 + 4 * cpr - 1)):
                    check_pair(rec_lib, b8, q8, 11, 6, src_h, src_w)
                    check_pair(rec_lib, q8, b8, 4, 16, src_h, src_w)
                    n += 2
    assert n > 4000


def test_lane_rows_without_a_division(rec_lib):
    for upr in range(1, 65):
        for ulps in (0, -1, 1):
            out = np.zeros((64, 5), np.int32)
            rec_lib.rec_lane_forms(upr, ulps, out.ctypes.data)
            lanes = np.arange(64)
            assert np.array_equal(out[:, 0], lanes // upr) and np.array_equal(out[:, 1], lanes % upr)
            assert np.array_equal(out[:, 2], out[:, 0]), upr  # the record's magic
            if upr <= 48:  # (raw_lanes_upr's bound: 0.5 / 48 away from every integer)
                assert np.array_equal(out[:, 3], out[:, 0]), (upr, ulps)  # the fp32 form the other kernels keep
                assert (out[:, 4] == 64 // upr).all(), (upr, ulps)


def test_rounding_trick_bias_identities():
    """For every 32 x in [0, 2^20) at every 1/128 step: the float path's bits (value + 1.5 * 2^23) against the subtracting form."""
    origins = np.array([0, 4, 1000, 32764], np.int64)
    seen = 0
    step = 1 << 22
    for lo in range(0, 1 << 27, step):
        v = (np.arange(lo, lo + step, dtype=np.int64).astype(np.float64) / 128.0).astype(np.float32)  # (rounded to float32 where 1/128 is below its resolution: every value the path can see)
        bits = (v + np.float32(12582912.0)).view(np.int32).astype(np.int64)
        sx = bits - BIAS
        assert (sx >= 0).all() and (sx <= 1 << 20).all()
        assert np.array_equal(bits & 31, sx & 31)
        assert np.array_equal(bits >> 5, (sx >> 5) + (BIAS >> 5))
        for x0 in origins:
            assert np.array_equal((bits >> 5) - (x0 + (BIAS >> 5)), (sx >> 5) - x0)
        seen += len(v)
    assert seen == 1 << 27


@pytest.mark.parametrize("x0,y0,cpr", [(0, 0, 1), (4, 1, 3), (1000, 777, 12), (4092, 4090, 40), (32000, 32700, 64), (32764, 0, 5), (0, 32766, 64)])
def test_tap_addresses_from_biased_coordinates(rec_lib, x0, y0, cpr):
    """mirror_rec_tap (a 24-bit multiply of the biased row, the biased origin folded into one constant) against
    ((sy >> 5) - y0) * pitch + 3 * ((sx >> 5) - x0), for every coordinate from the box origin to 2^20"""
    assert rec_lib.rec_tap_sweep(x0, y0, cpr) == 0
