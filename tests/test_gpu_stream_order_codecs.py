"""Everything else that takes a stream, held to stream order on a busy stream (tests/stream_order.py states the construction): the PNG
and JPEG encoders, the JPEG decoders, the lossless transcoder and composer, feature detection and matching, the circle fit, and one
pipeline decode -> remap -> encode on a single stalled stream.

The encoders, ``v1c_fit_circle`` and the decoders synchronise inside, so they are not asked to come back early; they are held to the
input that only arrives on the stream behind the stall (the encoders, the fit) and to a consumer on the stream of what they leave
queued (the decoders: the pixel stage runs behind the call's last synchronisation, the output buffer holds poison before it and is
overwritten right after the consumer).  ``v1c_jpeg_transcode`` / ``v1c_jpeg_compose`` read host files: they are held to running on a
stalled stream and leaving it usable.  Expected values: png_ref, jpg_ref / jpg_opt_ref, jpgdec_ref / jpgprog_ref, jpgxc_ref / jpgxf_ref,
feat_ref, circle_ref through the ``*_cases`` modules -- never an unstalled run of the product."""
import ctypes as C

import numpy as np
import pytest
import torch

import chainspecs as CS
import circle_cases as CC
import feat_ref as FR
import jpg_opt_cases as OC
import jpg_ref as JR
import jpgdec_cases as DC
import jpgprog_cases as PCS
import jpgxc_cases as XC
import jpgxf_cases as XF
import png_cases as NC
import png_ref as NR
import stream_order as SO
from test_gpu_codec_threads import Report, _shape_of, feature_pair, first_difference, job_compose, job_deflate, job_transcode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    import vr180_convert_amd as V

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    return V


@pytest.fixture(scope="module")
def lib(V):
    from vr180_convert_amd import _native

    return _native.lib()


@pytest.fixture(scope="module", autouse=True)
def _the_construction_bites(V, oracle_mod):
    SO.control(oracle_mod)


@pytest.fixture(scope="module")
def S():
    return torch.cuda.Stream()


def other(a, seed):
    """a decoy for ``a``: noise of its shape and type"""
    rng = np.random.default_rng(seed)
    hi = 256 if a.dtype == np.uint8 else 65536
    return rng.integers(0, hi, a.shape).astype(a.dtype)


def late(S, true, decoy, fn, check):
    """``fn(srcs)`` on the stalled stream with the true inputs arriving behind the stall; the buffers go back to the decoys right after.
    Twice on the same buffers -- cold, after ``clear_caches()``, and warm, whatever the suite ran before --, ``check(result)`` each time"""
    from vr180_convert_amd import remapper

    held, box = SO.Held(true, decoy), {}

    def call(srcs, dsts):
        box["got"] = fn(srcs)
        return []

    remapper.clear_caches()
    for _ in ("cold", "warm"):
        box.clear()
        held.run(S, call, launch_only=False)
        check(box["got"])


def usable(S):
    """the stream still orders work after the call"""
    with torch.cuda.stream(S):
        t = torch.arange(64, device="cuda")
        u = t * 2
    S.synchronize()
    assert u.sum().item() == 64 * 63


# ---- the encoders ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rows", [("runs_stride257_1row", 4), ("runs_gray16_stride257", 5)], ids=["uint8", "uint16"])
def test_png_deflate(lib, S, name, rows):
    """two bands, the second shorter"""
    img = NC.shared_cases()[name][0]
    assert rows < img.shape[0] <= 2 * rows
    want_segs, want_bands = NR.deflate(img, filter="paeth", band_rows=rows)
    assert len(want_bands) == 2
    def check(got):
        rc, segs, bands = got
        assert rc == 0, lib.v1c_last_error()
        assert bands == want_bands and segs == want_segs, first_difference(segs, want_segs)

    late(S, [img], [other(img, 1)], lambda srcs: job_deflate(img, srcs[0], "paeth", rows)(lib, S), check)


def _view(c, base):
    return torch.as_strided(base, (c.h, c.w, c.cn), (c.pitch, c.cn, 1), c.offset)


def _kw(c, **more):
    return {"quality": c.quality, "subsampling": c.subsampling, "restart_mcus": c.restart, **more}


@pytest.mark.parametrize("optimize", [False, True], ids=["v1c_jpeg_encode", "v1c_jpeg_encode_opt"])
def test_jpeg_encode(V, S, optimize):
    name = "restart1_17x9"
    c = OC.shared_cases()[name]
    want = OC.reference(name)[2 if optimize else 3]
    def check(got):
        assert got == want, first_difference(got, want)

    late(S, [c.base], [other(c.base, 2)], lambda srcs: V.encode_jpeg_tensor(_view(c, srcs[0]), **_kw(c, optimize=optimize)), check)


@pytest.mark.parametrize("optimize", [False, (True, False, True)], ids=["v1c_jpeg_encode_batch", "v1c_jpeg_encode_batch_opt"])
def test_jpeg_encode_batch(V, S, optimize):
    """three images of different sizes and channel counts in one list; with tables of their own for two of them"""
    names = ["noise_16x16_420", "bgra", OC.FLAT]
    cases = [OC.shared_cases()[n] for n in names]
    opts = [bool(optimize)] * 3 if isinstance(optimize, bool) else list(optimize)
    want = [OC.reference(n)[2 if o else 3] for n, o in zip(names, opts)]
    kw = {"quality": [c.quality for c in cases], "subsampling": [c.subsampling for c in cases], "restart_mcus": [c.restart for c in cases]}
    def check(got):
        assert V.last_encode_batch_report()["chunks"] == 1
        for n, g, w in zip(names, got, want):
            assert g == w, (n, first_difference(g, w))

    late(S, [c.base for c in cases], [other(c.base, 3 + k) for k, c in enumerate(cases)],
         lambda srcs: V.encode_jpeg_tensors([_view(c, b) for c, b in zip(cases, srcs)], optimize=opts, **kw), check)


# ---- the decoders: what stays queued behind the call's last synchronisation ------------------------------------------------------------
def _decoded(S, shapes, call):
    """the decoder's output buffers hold poison before the call; a consumer on the stream copies them, and they are overwritten at once"""
    held = SO.Held([], [], [(s, torch.uint8) for s in shapes])
    box = {}

    def run(srcs, dsts):
        box["rc"] = call(dsts)
        return dsts

    got, _ = held.run(S, run, launch_only=False)
    return box["rc"], got


@pytest.mark.parametrize("name,bits", [("size_17x17_420", 256), ("dri1_444", 0)])
def test_jpeg_decode(lib, S, name, bits):
    data = DC.supported_cases()[name]
    want = DC.reference(name, bits)
    rep = Report()
    rc, got = _decoded(S, [_shape_of(lib, data)], lambda o: lib.v1c_jpeg_decode(0, S.cuda_stream, data, len(data), o[0].data_ptr(), o[0].stride(0), 3, bits,
                                                                                C.byref(rep)))
    assert rc == 0, lib.v1c_last_error()
    assert got[0].tobytes() == want.pixels.tobytes() and (rep.segments, rep.subsequences) == (want.segments, want.subsequences)


def test_jpeg_decode_batch(lib, S):
    names = ("size_17x17_420", "dri1_444", "size_8x8_444")
    files = [DC.supported_cases()[n] for n in names]
    n = len(files)
    status, reports, rounds = (C.c_int * n)(*([7] * n)), (Report * n)(), C.c_uint32(0)

    def call(outs):
        data = (C.c_char_p * n)(*files)
        sizes = (C.c_uint64 * n)(*[len(f) for f in files])
        ptrs = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        pitches = (C.c_int64 * n)(*[o.stride(0) for o in outs])
        cns = (C.c_int * n)(*([3] * n))
        return lib.v1c_jpeg_decode_batch(0, S.cuda_stream, n, data, sizes, ptrs, pitches, cns, 256, 0, status, reports, C.byref(rounds))

    rc, got = _decoded(S, [_shape_of(lib, f) for f in files], call)
    assert rc == 0 and list(status) == [0] * n, (rc, list(status), lib.v1c_last_error())
    for name, g in zip(names, got):
        assert g.tobytes() == DC.reference(name, 256).pixels.tobytes(), name


def test_jpeg_prog_decode(lib, S):
    from vr180_convert_amd import _abi

    name = "pil_13x17_420"
    data = PCS.supported_cases()[name]
    info = _abi.JpegProgInfo()
    assert lib.v1c_jpeg_prog_info(data, len(data), C.byref(info)) == 0, lib.v1c_last_error()
    rep, per = _abi.JpegProgReport(), (C.c_uint32 * info.scans)()
    rc, got = _decoded(S, [(info.height, info.width, 3)], lambda o: lib.v1c_jpeg_prog_decode(
        0, S.cuda_stream, data, len(data), o[0].data_ptr(), o[0].stride(0), 3, 256, C.byref(rep), per, info.scans))
    assert rc == 0, lib.v1c_last_error()
    want = PCS.reference(name, 256)
    assert got[0].tobytes() == want.pixels.tobytes() and list(per) == list(want.scan_rounds)


# ---- host files in, host files out: run on a stalled stream, leave it usable ------------------------------------------------------------
def test_jpeg_transcode_on_a_stalled_stream(lib, S):
    name = "swap_2x2_420"
    SO.stall(S)
    rc, _, _, _, files = job_transcode(*XC.cases()[name])(lib, S)
    assert rc == 0, lib.v1c_last_error()
    assert tuple(files) == XC.reference(name)
    usable(S)


def test_jpeg_compose_on_a_stalled_stream(lib, S):
    name = "mixed_transpose_symmetric_tables"  # (a rot90 region beside a flipped one of another file)
    SO.stall(S)
    rc, _, files = job_compose(*XF.cases()[name])(lib, S)
    assert rc == 0, lib.v1c_last_error()
    assert tuple(files) == XF.reference(name)
    usable(S)


# ---- features: detect, detect, match behind one stall ------------------------------------------------------------------------------------
def test_feature_detect_then_match_without_a_host_step(lib, S):
    """Both detections and the match are queued on the stream behind ONE stall, on images that arrive late; nothing goes to the host in
    between.  ``v1c_feat_match`` takes its descriptor counts as host arguments: they are the restatement's here (where the product reads
    the detections' counts back first), and the detections' device counts are held to them afterwards."""
    from vr180_convert_amd import features as F

    a, b = feature_pair()
    (k1, d1), (k2, d2) = FR.detect(a, radius=48.0), FR.detect(b, radius=48.0)
    i1, i2, dist = FR.match(d1, d2)
    assert len(k1) > 8 and len(k2) > 8 and len(i1) > 4
    p = F.params(1.0, 48.0)
    held = SO.Held([a, b], [other(a, 7), other(b, 8)])

    def call(srcs, dsts):
        ka, da, ca = F._detect_enqueue(srcs[0], p)
        kb, db, cb = F._detect_enqueue(srcs[1], p)
        pairs, dd, cm = F._match_enqueue(da[:len(d1)], db[:len(d2)], p)
        return [ka[:len(k1)], da[:len(d1)], ca, kb[:len(k2)], db[:len(d2)], cb, pairs, dd, cm]

    for run in range(2):
        got, queued = held.run(S, call, launch_only=False)  # (v1c_feat_detect may wait for its pageable copy: the header's exception)
        print(f"detect, detect, match run {run}: back with the stall {'still pending' if queued else 'over'}")
        ka, da, ca, kb, db, cb, pairs, dd, cm = got
        assert (int(ca[0]), int(cb[0]), int(cm[0])) == (len(k1), len(k2), len(i1)), run
        assert np.array_equal(ka, k1.astype(np.int32)) and np.array_equal(da, d1.astype(np.uint8)), run
        assert np.array_equal(kb, k2.astype(np.int32)) and np.array_equal(db, d2.astype(np.uint8)), run
        m = len(i1)
        assert np.array_equal(pairs[:m], np.stack([i1, i2], axis=1).astype(np.int32)) and np.array_equal(dd[:m], dist.astype(np.int32)), run


def test_feature_match_is_launch_only(S):
    """``v1c_feat_match`` alone, on descriptors that arrive behind the stall: the header calls it launch-only, so the warm call must be
    back with the stall still in force (its scratch is allocated and freed in stream order)"""
    from vr180_convert_amd import features as F

    a, b = feature_pair()
    d1, d2 = (np.ascontiguousarray(FR.detect(im, radius=48.0)[1].astype(np.uint8)) for im in (a, b))
    i1, i2, dist = FR.match(d1, d2)
    assert len(i1) > 4
    p = F.params(1.0, 48.0)
    held = SO.Held([d1, d2], [other(d1, 9), other(d2, 10)])
    for run in range(2):
        got, _ = held.run(S, lambda srcs, dsts: F._match_enqueue(srcs[0], srcs[1], p), launch_only=run == 1)
        pairs, dd, cm = got
        m = len(i1)
        assert int(cm[0]) == m, run
        assert np.array_equal(pairs[:m], np.stack([i1, i2], axis=1).astype(np.int32)) and np.array_equal(dd[:m], dist.astype(np.int32)), run


# ---- the circle fit ----------------------------------------------------------------------------------------------------------------------
def _same_doubles(got, want, what):
    assert list(got[3:6]) == list(want[3:6]) and got[7] == 0, (what, got, want)
    assert np.abs(got[[0, 1, 2, 6]] - want[[0, 1, 2, 6]]).max() <= 1e-9, (what, got, want)  # (the bound of tests/test_gpu_circle.py)


def test_fit_circle_async_with_a_poisoned_workspace(lib, S):
    """launch-only: four launches on a workspace that holds poison before the stall, the image arriving behind it"""
    from vr180_convert_amd import circle

    true, decoy = CC.shared_cases()["aa_disc_1"].img, CC.shared_cases()["aa_disc_2"].img
    assert true.shape == decoy.shape
    h, w, cn = true.shape
    held = SO.Held([np.ascontiguousarray(true)], [np.ascontiguousarray(decoy)],
                   [((int(lib.v1c_fit_circle_workspace(h, w)),), torch.uint8), ((8,), torch.float64)])
    p = circle.params()

    def call(srcs, dsts):
        rc = lib.v1c_fit_circle_async(0, S.cuda_stream, srcs[0].data_ptr(), h, w, w * cn, cn, 0, C.byref(p), dsts[0].data_ptr(), dsts[1].data_ptr())
        assert rc == 0, lib.v1c_last_error()
        return [dsts[1]]

    for run in range(2):
        got, _ = held.run(S, call, launch_only=run == 1)
        _same_doubles(got[0], CC.reference("aa_disc_1")[0], run)


def test_fit_circle_synchronous(S):
    from vr180_convert_amd import circle

    true, decoy = CC.shared_cases()["aa_disc_1"].img, CC.shared_cases()["aa_disc_2"].img
    want, want_rim = CC.reference("aa_disc_1")

    def check(got):
        assert np.array_equal(got[1], want_rim)
        _same_doubles(got[0], want, "v1c_fit_circle")

    late(S, [np.ascontiguousarray(true)], [np.ascontiguousarray(decoy)], lambda srcs: circle.fit_circle_raw(srcs[0], points=True), check)


# ---- one pipeline on one stalled stream ----------------------------------------------------------------------------------------------------
def test_decode_remap_encode_on_one_stalled_stream(V, oracle_mod, S):
    """a side-by-side JPEG file is decoded, its halves remapped into a side-by-side result and that encoded, all on a stream that was
    busy when the first call was made and with no synchronisation of the test's own before the file is there; once cold (the remap's
    plan is created inside the pipeline) and once warm"""
    from vr180_convert_amd import remapper

    name = "noise_q100_420"  # 64 x 96: two eyes of 64 x 48
    data = DC.supported_cases()[name]
    spec = [("equirect_enc", True), CS.EQUI]
    restart = JR.default_restart_mcus(64, 128, 3, "420")
    px = DC.reference(name).pixels
    assert px.shape == (64, 96, 3)
    want_img = oracle_mod.apply_lr(spec, np.ascontiguousarray(px[:, :48]), np.ascontiguousarray(px[:, 48:]), size_output=(64, 64), interpolation=1,
                                   radius=24.0)
    want = JR.encode(want_img, 95, "420", restart)
    remapper.clear_caches()
    for run in ("cold", "warm"):
        with torch.cuda.stream(S):
            SO.stall(S)
            sbs = V.decode_jpeg_tensor(data)
            out = V.apply_lr_tensors(CS.to_product(spec), sbs[:, :48], sbs[:, 48:], size_output=(64, 64), interpolation=1, radius=24.0)
            got = V.encode_jpeg_tensor(out, quality=95, subsampling="420", restart_mcus=restart)
            SO.poison(sbs)
            SO.poison(out)
        S.synchronize()
        assert got == want, (run, first_difference(got, want))
