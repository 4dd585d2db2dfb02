"""The device codecs under concurrent threads on the MI355X.  Every other test of the codecs runs on one thread; here one process runs
them from up to four threads at once, each with a stream of its own, and holds every result byte for byte to what the same call gives
serially -- the values the other tests hold to the restatements.

(a) the C ABI: a table of engine calls with buffers of their own, run rotated from four threads.  The entries take their workspaces per
    call, the decoders take turns at their staging buffer, ``v1c_last_error`` is per thread: this is where that is exercised.
(b) the Python layer under a FIXED interleaving: thread A's engine call returns, thread B runs a whole call, then A reads its result.
    A page-locked result buffer shared between threads hands A the bytes of B; this schedule shows it every time, without luck.  The
    ``last_*_report()`` functions are held to the calling thread's call by the same schedule.
(c) the Python layer under plain concurrency: the soak half of (b), which may pass by luck where (b) cannot.

The waits (5 s, 120 s) only turn a stall into a failure; nothing here rests on a measured time."""
import ctypes as C
import threading
import time

import numpy as np
import pytest
import torch

import analytic_ref as A
import feat_ref as FR
import jpg_cases as PC
import jpg_opt_cases as OC
import jpg_ref as R
import jpgdec_cases as DC
import jpgprog_cases as PCS
import jpgxc_cases as XC
import jpgxf_cases as XF
import png_cases as NC
import png_ref as NR

pytestmark = pytest.mark.gpu

THREADS = 4          # the hardware queues a process gets here
JOIN_TIMEOUT = 120   # seconds until a thread that has not come back fails the test
HANDOVER = 5         # seconds thread A waits for B in the fixed interleaving: a fix that takes turns with a lock lets B run behind A
_STALLED: list = []  # names of threads a test of this file left running


class Report(C.Structure):
    _fields_ = [("segments", C.c_uint32), ("subsequences", C.c_uint32), ("rounds", C.c_uint32), ("reserved", C.c_uint32),
                ("error_pos", C.c_uint64)]


@pytest.fixture(autouse=True)
def _nothing_left_running():
    if _STALLED:
        pytest.fail(f"an earlier test of this file left {_STALLED} running: no further GPU work is started")


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


def run_threads(targets: dict) -> dict:
    """every ``targets[name](stream)`` on a thread of that name, inside a stream of its own; the results by name.  A thread that is not
    back after JOIN_TIMEOUT fails the test with its name, an exception in a thread is raised here."""
    assert len(targets) <= THREADS and not _STALLED
    results, errors = {}, {}

    def body(name, fn):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                results[name] = fn(s)
                s.synchronize()
        except BaseException as e:  # noqa: BLE001 - raised again on the test's thread
            errors[name] = e

    threads = [threading.Thread(target=body, args=(n, f), name=n, daemon=True) for n, f in targets.items()]
    torch.cuda.synchronize()  # (the inputs: uploaded on the test thread's stream)
    for t in threads:
        t.start()
    deadline = time.monotonic() + JOIN_TIMEOUT
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    alive = [t.name for t in threads if t.is_alive()]
    if alive:
        _STALLED.extend(alive)
        pytest.fail(f"threads {alive} still alive {JOIN_TIMEOUT} s after their start")
    for name in targets:
        if name in errors:
            raise errors[name]
    return results


def first_difference(a: bytes, b: bytes):
    return len(a), len(b), next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)


# ---- (a) the C ABI ---------------------------------------------------------------------------------------------------------------------
ENCODE, ENCODE_OPT, DEFLATE16 = "noise_q100_420", "gray_136_q95_r1", "runs_gray16_stride257"
BATCH_OPT = (("noise_16x16_420", True), ("bgra", False), ("gray_136_q100", True))  # (case of jpg_opt_cases, optimize)
DECODE_256, DECODE_0, DECODE_BATCH, PROGRESSIVE = "noise_q100_422", "dri1_444", ("size_17x17_420", "dri1_gray", "noise_q100_444"), "pil_13x17_420"
TRANSCODE, COMPOSE = "swap_dri7_420", "mixed_transpose_symmetric_tables"  # (the latter: a rot90 region beside a flipped one of another file)
DEFLATE_ROWS = 2


def feature_pair():
    """a 96 x 96 noise disc and itself two pixels to the right"""
    a = A.noise(np.uint8, 96, 96, 3, 5)
    y, x = np.mgrid[:96, :96]
    a[(x - 47.5) ** 2 + (y - 47.5) ** 2 > 48.0 ** 2] = 0
    return a, np.roll(a, 2, axis=1)


def _encode_args(c, base):
    return (base.data_ptr() + c.offset, c.h, c.w, c.pitch, c.cn, c.quality, R.SUBSAMPLINGS[c.subsampling], c.restart)


def job_encode(c, base):
    def run(lib, stream):
        args = _encode_args(c, base)
        cap = int(lib.v1c_jpeg_bound(c.h, c.w, c.cn, args[6], c.restart))
        out, size = np.full(cap, 0xA5, np.uint8), C.c_uint64(0)
        rc = lib.v1c_jpeg_encode(0, stream.cuda_stream, *args, out.ctypes.data, cap, C.byref(size))
        return rc, out[:size.value].tobytes()
    return run


def job_encode_opt(c, base):
    from vr180_convert_amd.jpeg_device import DHT_MAX

    def run(lib, stream):
        args = _encode_args(c, base)
        cap = int(lib.v1c_jpeg_bound(c.h, c.w, c.cn, args[6], c.restart))
        out, size = np.full(cap, 0xA5, np.uint8), C.c_uint64(0)
        dht, dht_size = (C.c_uint8 * DHT_MAX)(), C.c_uint32(0)
        rc = lib.v1c_jpeg_encode_opt(0, stream.cuda_stream, *args, out.ctypes.data, cap, C.byref(size), dht, C.byref(dht_size))
        return rc, out[:size.value].tobytes(), bytes(dht[:dht_size.value])
    return run


def job_encode_batch_opt(members):
    """members: (case, its buffer on the device, optimize)"""
    from vr180_convert_amd.jpeg_device import JpegImageOpt

    def run(lib, stream):
        bounds = [int(lib.v1c_jpeg_bound(c.h, c.w, c.cn, R.SUBSAMPLINGS[c.subsampling], c.restart)) for c, _, _ in members]
        out = np.full(sum(bounds), 0xA5, np.uint8)
        images = (JpegImageOpt * len(members))()
        at = 0
        for k, ((c, base, opt), b) in enumerate(zip(members, bounds)):
            images[k] = JpegImageOpt(*_encode_args(c, base), out.ctypes.data + at, b, 0, int(opt))
            at += b
        chunks = C.c_uint32(0)
        rc = lib.v1c_jpeg_encode_batch_opt(0, stream.cuda_stream, len(members), images, 0, C.byref(chunks))
        files, at = [], 0
        for im, b in zip(images, bounds):
            files.append((out[at:at + int(im.size)].tobytes(), bytes(im.dht[:im.dht_size])))
            at += b
        return rc, chunks.value, files
    return run


def job_deflate(img, t, filter, rows):
    from vr180_convert_amd import _abi
    from vr180_convert_amd.png_device import FILTERS, Band

    h, w, cn = img.shape
    depth = _abi.DEPTH_16U if img.itemsize == 2 else _abi.DEPTH_8U

    def run(lib, stream):
        cap = int(lib.v1c_png_bound(h, w, cn, depth, rows))
        out = np.full(cap, 0xA5, np.uint8)
        bands = (Band * (-(-h // min(rows, h))))()
        count, size = C.c_int32(0), C.c_uint64(0)
        rc = lib.v1c_png_deflate(0, stream.cuda_stream, t.data_ptr(), h, w, w * cn * img.itemsize, cn, depth, FILTERS[filter], rows, out.ctypes.data,
                                 cap, bands, C.byref(count), C.byref(size))
        return rc, out[:size.value].tobytes(), [(b.row0, b.row1, b.offset, b.size, b.adler32, b.stored) for b in bands[:count.value]]
    return run


def _shape_of(lib, data):
    from vr180_convert_amd.jpeg_decode_device import _Info

    info = _Info()
    assert lib.v1c_jpeg_decode_info(data, len(data), C.byref(info)) == 0, lib.v1c_last_error()
    return info.height, info.width, 3


def job_decode(data, S, shape):
    def run(lib, stream):
        out = torch.full(shape, 0xA5, dtype=torch.uint8, device="cuda")
        rep = Report()
        rc = lib.v1c_jpeg_decode(0, stream.cuda_stream, data, len(data), out.data_ptr(), out.stride(0), 3, S, C.byref(rep))
        return rc, rep.segments, rep.subsequences, rep.rounds, out.cpu().numpy().tobytes()  # (the pixel stage is queued: .cpu() waits for it)
    return run


def job_decode_fails(data, S, shape):
    """a damaged file: the code and what the calling thread is told"""
    def run(lib, stream):
        out = torch.zeros(shape, dtype=torch.uint8, device="cuda")
        rc = lib.v1c_jpeg_decode(0, stream.cuda_stream, data, len(data), out.data_ptr(), out.stride(0), 3, S, None)
        return rc, lib.v1c_last_error()
    return run


def job_decode_batch(files, shapes, S):
    def run(lib, stream):
        n = len(files)
        outs = [torch.full(s, 0xA5, dtype=torch.uint8, device="cuda") for s in shapes]
        data = (C.c_char_p * n)(*files)
        sizes = (C.c_uint64 * n)(*[len(f) for f in files])
        ptrs = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        pitches = (C.c_int64 * n)(*[o.stride(0) for o in outs])
        cns = (C.c_int * n)(*([3] * n))
        status, reports, rounds = (C.c_int * n)(*([7] * n)), (Report * n)(), C.c_uint32(0)
        rc = lib.v1c_jpeg_decode_batch(0, stream.cuda_stream, n, data, sizes, ptrs, pitches, cns, S, 0, status, reports, C.byref(rounds))
        return (rc, rounds.value, list(status), [(r.segments, r.subsequences, r.rounds) for r in reports],
                [o.cpu().numpy().tobytes() for o in outs])
    return run


def job_prog_decode(data, S):
    from vr180_convert_amd import _abi

    def run(lib, stream):
        info = _abi.JpegProgInfo()
        assert lib.v1c_jpeg_prog_info(data, len(data), C.byref(info)) == 0, lib.v1c_last_error()
        out = torch.full((info.height, info.width, 3), 0xA5, dtype=torch.uint8, device="cuda")
        rep, per = _abi.JpegProgReport(), (C.c_uint32 * info.scans)()
        rc = lib.v1c_jpeg_prog_decode(0, stream.cuda_stream, data, len(data), out.data_ptr(), out.stride(0), 3, S, C.byref(rep), per, info.scans)
        return rc, rep.scans, rep.segments, rep.subsequences, rep.rounds, list(per), out.cpu().numpy().tobytes()
    return run


def _lossless_outputs(kind, region, specs, mcu_width):
    """the ``v1c_jpeg_xc_output`` / ``v1c_jpeg_xf_output`` array of a case's outputs (regions with numbers only), and what it points to"""
    outs, keep = (kind * len(specs))(), []
    for o, spec in zip(outs, specs):
        arr = (region * len(spec["regions"]))(*[region(*r) for r in spec["regions"]])
        keep.append(arr)
        r = spec.get("restart_mcus")
        o.width, o.height = spec["width"], spec["height"]
        o.restart_mcus = min(65535, -(-spec["width"] // mcu_width)) if r is None else r
        o.optimize, o.nregions, o.regions = int(bool(spec.get("optimize"))), len(spec["regions"]), arr
    return outs, keep


def _carve(outs, bounds):
    buf = np.full(sum(bounds), 0xA5, np.uint8)
    at = 0
    for o, b in zip(outs, bounds):
        o.out_host, o.capacity = buf.ctypes.data + at, b
        at += b
    return buf


def _files(outs, bounds, buf, header):
    files, at = [], 0
    for o, b in zip(outs, bounds):
        head = (C.c_uint8 * 2048)()
        n = header(o, head)
        assert n > 0
        files.append(bytes(head[:n]) + buf[at:at + int(o.size)].tobytes() + b"\xff\xd9")
        assert (buf[at + int(o.size):at + b] == 0xA5).all()  # nothing behind the scan is written
        at += b
    return files


def job_transcode(data, specs):
    from vr180_convert_amd.jpeg_transcode_device import XcOutput, XcRegion, probe_mcu

    mw = probe_mcu(data)[2]

    def run(lib, stream):
        outs, keep = _lossless_outputs(XcOutput, XcRegion, specs, mw)
        bounds = [max(int(lib.v1c_jpeg_transcode_bound(data, len(data), o.width, o.height, o.restart_mcus)), 1 << 12) for o in outs]
        buf, rep = _carve(outs, bounds), Report()
        rc = lib.v1c_jpeg_transcode(0, stream.cuda_stream, data, len(data), len(specs), outs, 0, C.byref(rep))
        files = [] if rc else _files(outs, bounds, buf, lambda o, head: lib.v1c_jpeg_header_xc(
            data, len(data), o.width, o.height, o.restart_mcus, o.dht if o.optimize else None, o.dht_size, head, 2048))
        return rc, rep.segments, rep.subsequences, rep.rounds, files
    return run


def job_compose(datas, specs):
    from vr180_convert_amd.jpeg_compose_device import XfOutput, XfRegion, XfSource
    from vr180_convert_amd.jpeg_transcode_device import probe_mcu

    mw = probe_mcu(datas[0])[2]
    assert all(isinstance(r[1], int) for spec in specs for r in spec["regions"])

    def run(lib, stream):
        srcs = (XfSource * len(datas))(*[XfSource(d, len(d)) for d in datas])
        outs, keep = _lossless_outputs(XfOutput, XfRegion, specs, mw)
        d0 = datas[0]
        bounds = [max(int(lib.v1c_jpeg_compose_bound(d0, len(d0), o.width, o.height, o.restart_mcus)), 1 << 12) for o in outs]
        buf, reps = _carve(outs, bounds), (Report * len(datas))()
        rc = lib.v1c_jpeg_compose(0, stream.cuda_stream, len(datas), srcs, len(specs), outs, 0, reps)
        first = iter([spec["regions"][0][:2] for spec in specs])  # (region 0's file and transform: whose tables the output has)

        def header(o, head):
            si, code = next(first)
            return lib.v1c_jpeg_header_xf(datas[si], len(datas[si]), o.width, o.height, o.restart_mcus, code >> 2, o.dht if o.optimize else None,
                                          o.dht_size, head, 2048)

        files = [] if rc else _files(outs, bounds, buf, header)
        return rc, [(r.segments, r.subsequences, r.rounds) for r in reps], files
    return run


def job_features(t1, t2):
    """the detect entry on both images, then the match entry on what it found: keypoints, descriptors, pairs and distances"""
    from vr180_convert_amd import features as F

    p = F.params(1.0, 48.0)

    def run(lib, stream):
        found = []
        for t in (t1, t2):
            kp = torch.zeros((p.max_keypoints, len(F.KP_FIELDS)), dtype=torch.int32, device="cuda")
            desc = torch.zeros((p.max_keypoints, 32), dtype=torch.uint8, device="cuda")
            count = torch.zeros(1, dtype=torch.int32, device="cuda")
            rc = lib.v1c_feat_detect(0, stream.cuda_stream, t.data_ptr(), t.shape[0], t.shape[1], t.stride(0), t.shape[2], C.byref(p), kp.data_ptr(),
                                     desc.data_ptr(), count.data_ptr())
            if rc:
                return rc, lib.v1c_last_error()
            n = int(count.cpu()[0])
            found.append((kp[:n], desc[:n]))
        (k1, d1), (k2, d2) = found
        cap = max(1, min(len(d1), len(d2)))
        pairs = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
        dist = torch.zeros(cap, dtype=torch.int32, device="cuda")
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        rc = lib.v1c_feat_match(0, stream.cuda_stream, d1.data_ptr() if len(d1) else None, len(d1), d2.data_ptr() if len(d2) else None, len(d2),
                                C.byref(p), pairs.data_ptr(), dist.data_ptr(), count.data_ptr())
        m = int(count.cpu()[0])
        return (rc, *[x.cpu().numpy().tobytes() for x in (k1, d1, k2, d2, pairs[:m], dist[:m])])
    return run


@pytest.fixture(scope="module")
def table(lib):
    """name: job.  A job is a closure over (lib, stream) that makes one engine call -- the feature job three -- with buffers of its own"""
    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    jobs = {}
    c = PC.shared_cases()[ENCODE]
    assert (c.cn, c.subsampling) == (3, "420")
    jobs["encode"] = job_encode(c, up(c.base))
    c = OC.shared_cases()[ENCODE_OPT]
    assert c.cn == 1
    jobs["encode_opt"] = job_encode_opt(c, up(c.base))
    members = [(OC.shared_cases()[n], up(OC.shared_cases()[n].base), o) for n, o in BATCH_OPT]
    assert len({(m[0].h, m[0].w) for m in members}) == 3 and {m[2] for m in members} == {True, False}
    jobs["encode_batch_opt"] = job_encode_batch_opt(members)
    img = NC.shared_cases()[DEFLATE16][0]
    assert img.dtype == np.uint16 and img.shape[0] > 2 * DEFLATE_ROWS and img.shape[0] % DEFLATE_ROWS
    jobs["png_deflate"] = job_deflate(img, up(img), "paeth", DEFLATE_ROWS)
    files = DC.supported_cases()
    jobs["decode_256"] = job_decode(files[DECODE_256], 256, _shape_of(lib, files[DECODE_256]))
    jobs["decode_0"] = job_decode(files[DECODE_0], 0, _shape_of(lib, files[DECODE_0]))
    jobs["decode_batch"] = job_decode_batch([files[n] for n in DECODE_BATCH], [_shape_of(lib, files[n]) for n in DECODE_BATCH], 256)
    jobs["prog_decode"] = job_prog_decode(PCS.supported_cases()[PROGRESSIVE], 256)
    jobs["transcode"] = job_transcode(*XC.cases()[TRANSCODE])
    jobs["compose"] = job_compose(*XF.cases()[COMPOSE])
    a, b = feature_pair()
    jobs["features"] = job_features(up(a), up(b))
    torch.cuda.synchronize()
    return jobs


@pytest.fixture(scope="module")
def serial(lib, table):
    """every job once on the test's thread, on a stream of its own: the values the one-thread tests hold to the restatements"""
    s = torch.cuda.Stream()
    out = {}
    with torch.cuda.stream(s):
        for name, job in table.items():
            out[name] = job(lib, s)
            assert out[name][0] == 0, (name, lib.v1c_last_error())
    s.synchronize()
    return out


def test_serial_pass_equals_the_restatements(serial):
    """so that this file does not rest on the code under test alone: the cheapest jobs against jpg_ref, png_ref, the decoder's
    restatement and feat_ref"""
    c = PC.shared_cases()[ENCODE]
    data = PC.reference(ENCODE)[2]
    head = R.headers(R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart), c.quality)
    assert data.startswith(head) and serial["encode"][1] == data[len(head):-2], first_difference(serial["encode"][1], data[len(head):-2])

    segs, bands = NR.deflate(NC.shared_cases()[DEFLATE16][0], filter="paeth", band_rows=DEFLATE_ROWS)
    assert len(bands) > 2 and bands[-1][1] - bands[-1][0] < DEFLATE_ROWS  # (several bands, a shorter last one)
    assert serial["png_deflate"][2] == bands and serial["png_deflate"][1] == segs, first_difference(serial["png_deflate"][1], segs)

    want = DC.reference(DECODE_256, 256)
    _, segments, subsequences, rounds, pixels = serial["decode_256"]
    assert pixels == want.pixels.tobytes() and (segments, subsequences) == (want.segments, want.subsequences) and 1 <= rounds <= want.rounds

    a, b = feature_pair()
    (k1, d1), (k2, d2) = FR.detect(a, radius=48.0), FR.detect(b, radius=48.0)
    i1, i2, dist = FR.match(d1, d2)
    assert len(k1) > 8 and len(i1) > 4
    pairs = np.stack([i1, i2], axis=1).astype(np.int32)
    got = serial["features"][1:]
    want = [np.ascontiguousarray(x).tobytes() for x in (k1.astype(np.int32), d1.astype(np.uint8), k2.astype(np.int32), d2.astype(np.uint8), pairs,
                                                        dist.astype(np.int32))]
    assert [len(g) for g in got] == [len(w) for w in want] and got == tuple(want)


def test_c_abi_from_four_threads(lib, table, serial):
    """Thread k runs the table rotated by k, three times over, behind a barrier per round; every result -- bytes, codes, rounds,
    segments -- is the serial one.  Thread 0 decodes a truncated file among its jobs and the others make a call that is refused for an
    argument: each reads ITS message from ``v1c_last_error``, and every other call stays V1C_OK."""
    rounds = 3
    names = list(table)
    damaged = DC.corrupt_cases()[DC.TRUNCATED][0]
    fails = job_decode_fails(damaged, 256, _shape_of(lib, damaged))
    s0 = torch.cuda.Stream()
    with torch.cuda.stream(s0):
        want_failure = fails(lib, s0)
    assert want_failure[0] == -5 and b"damaged" in want_failure[1]
    scrap = (C.c_uint8 * 16)()  # (never written: the argument checks come first)
    refused = {1: (None, 3, 256, b"NULL"), 2: (C.addressof(scrap), 4, 256, b"out_cn"), 3: (C.addressof(scrap), 3, 100, b"subseq_bits")}  # out, out_cn, S
    barrier, stop, wrong = threading.Barrier(THREADS), threading.Event(), []

    def worker(k):
        def run(stream):
            try:
                for r in range(rounds):
                    barrier.wait(JOIN_TIMEOUT)
                    for j in range(len(names)):
                        if stop.is_set():
                            return
                        name = names[(j + k) % len(names)]
                        got = table[name](lib, stream)
                        if got != serial[name]:
                            wrong.append((k, r, name, got[0], lib.v1c_last_error() if got[0] else b""))
                            stop.set()
                            return
                        if j != len(names) // 2:
                            continue
                        if k == 0:  # a call that fails on the device ...
                            got = fails(lib, stream)
                            mine = got == want_failure
                        else:       # ... and calls that are refused for an argument before they reach it, each for another one
                            out, cn, S, word = refused[k]
                            got = lib.v1c_jpeg_decode(0, stream.cuda_stream, damaged, len(damaged), out, 0, cn, S, None), lib.v1c_last_error()
                            mine = got[0] == -1 and word in got[1]
                        if not mine:
                            wrong.append((k, r, "the failing call", got))
                            stop.set()
                            return
            except threading.BrokenBarrierError:  # (another thread stopped: what it found is in `wrong`, or it raises)
                return
            except BaseException:
                stop.set()
                raise
            finally:
                if stop.is_set():
                    barrier.abort()
        return run

    run_threads({f"abi-{k}": worker(k) for k in range(THREADS)})
    assert not wrong, wrong[:4]
    # and the engine is as it was: the whole table once more, serially
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for name in names:
            assert table[name](lib, s) == serial[name], name


# ---- (b) the Python layer under a fixed interleaving -----------------------------------------------------------------------------------
def interleave(monkeypatch, entry, call_a, call_b, report=None):
    """``call_a`` on thread A and ``call_b`` on thread B so that B's whole call lies between the return of A's first ``entry`` call -- an
    attribute of the engine's library object, replaced here by a Python callable that calls the real one -- and what A does with its
    result.  A waits HANDOVER seconds at the most, so callers that take turns with a lock pass too: B then runs behind A.  Returns both
    results; with ``report``, B makes its call once more after A's has come back, and ``report()`` as each thread then reads it is
    returned too."""
    from vr180_convert_amd import _native

    lib = _native.lib()
    real = getattr(lib, entry)
    a_returned, b_done, a_finished, b_finished = (threading.Event() for _ in range(4))
    state = {"a": None, "fired": False}

    def hooked(*args):
        rc = real(*args)
        if threading.get_ident() == state["a"] and not state["fired"]:
            state["fired"] = True
            a_returned.set()
            b_done.wait(HANDOVER)
        return rc

    monkeypatch.setattr(lib, entry, hooked)

    def run_a(stream):
        state["a"] = threading.get_ident()
        try:
            got = call_a()
        finally:
            a_returned.set()
            a_finished.set()
        if report is None:
            return got
        assert b_finished.wait(JOIN_TIMEOUT / 2)
        return got, report()

    def run_b(stream):
        try:
            assert a_returned.wait(JOIN_TIMEOUT / 2)
            try:
                got = call_b()
            finally:
                b_done.set()
            if report is None:
                return got
            assert a_finished.wait(JOIN_TIMEOUT / 2)
            assert call_b() == got
            return got, report()
        finally:
            b_done.set()
            b_finished.set()

    out = run_threads({"A": run_a, "B": run_b})
    assert state["fired"], f"{entry} was not called on thread A"
    return out["A"], out["B"]


def check_pair(monkeypatch, entry, call_a, call_b, longer_b=False):
    """both calls alone on the test's thread, then interleaved: the same results.  ``longer_b``: the call with the longer result is B"""
    want_a, want_b = call_a(), call_b()
    assert want_a != want_b
    if longer_b and len(want_b) < len(want_a):
        call_a, call_b, want_a, want_b = call_b, call_a, want_b, want_a
    got_a, got_b = interleave(monkeypatch, entry, call_a, call_b)
    assert got_b == want_b, ("B", first_difference(got_b, want_b) if isinstance(got_b, bytes) else None)
    assert got_a == want_a, ("A", first_difference(got_a, want_a) if isinstance(got_a, bytes) else None)


@pytest.fixture(scope="module")
def images(V):
    """noise images on the device: two of 64 x 64, one of 256 x 256, and three of mixed sizes for a batch"""
    shapes = {"a64": (64, 64, 1), "b64": (64, 64, 2), "c256": (256, 256, 3), "l0": (48, 64, 4), "l1": (56, 72, 5), "l2": (64, 48, 6),
              "m0": (72, 56, 7), "m1": (48, 80, 8)}
    out = {k: torch.from_numpy(A.noise(np.uint8, h, w, 3, seed)).cuda() for k, (h, w, seed) in shapes.items()}
    torch.cuda.synchronize()
    return out


SBS_420, SBS_444 = "noise_q100_420", "noise_q100_444"  # 96 x 64 files of the decoder's cases: halves of three and six MCUs


@pytest.mark.parametrize("optimize", [False, True], ids=["plain", "optimize"])
def test_two_encodes_of_one_size(V, images, monkeypatch, optimize):
    check_pair(monkeypatch, "v1c_jpeg_encode_opt" if optimize else "v1c_jpeg_encode",
               lambda: V.encode_jpeg_tensor(images["a64"], optimize=optimize), lambda: V.encode_jpeg_tensor(images["b64"], optimize=optimize), longer_b=True)


@pytest.mark.parametrize("a,b", [("a64", "c256"), ("c256", "a64")], ids=["small_then_large", "large_then_small"])
def test_two_encodes_of_two_sizes(V, images, monkeypatch, a, b):
    """both orders: the larger result replaces a buffer that is too small, the smaller one overwrites it"""
    check_pair(monkeypatch, "v1c_jpeg_encode", lambda: V.encode_jpeg_tensor(images[a]), lambda: V.encode_jpeg_tensor(images[b]))


def test_two_png_encodes(V, images, monkeypatch):
    from vr180_convert_amd import png_device as P

    check_pair(monkeypatch, "v1c_png_deflate", lambda: P.encode_png_tensor(images["a64"]), lambda: P.encode_png_tensor(images["b64"]), longer_b=True)


def test_batch_encode_and_single_encode(V, images, monkeypatch):
    check_pair(monkeypatch, "v1c_jpeg_encode_batch", lambda: V.encode_jpeg_tensors([images[k] for k in ("l0", "l1", "l2")]),
               lambda: V.encode_jpeg_tensor(images["c256"]))


def test_imwrite_and_single_encode(V, images, monkeypatch, tmp_path):
    """the scan goes from the page-locked buffer to the file without a copy in between: A's FILE is compared"""
    def write():
        V.imwrite_jpeg_tensor(tmp_path / "a.jpg", images["a64"])
        return (tmp_path / "a.jpg").read_bytes()

    check_pair(monkeypatch, "v1c_jpeg_encode", write, lambda: V.encode_jpeg_tensor(images["b64"]))


def test_split_and_single_encode(V, images, monkeypatch):
    """the lossless entries land in the encoder's buffer"""
    data = DC.supported_cases()[SBS_420]
    check_pair(monkeypatch, "v1c_jpeg_transcode", lambda: V.split_sbs_jpeg(data), lambda: V.encode_jpeg_tensor(images["c256"]))


def test_rotate_and_swap(V, monkeypatch):
    files = DC.supported_cases()
    check_pair(monkeypatch, "v1c_jpeg_compose", lambda: V.transform_jpeg(files[SBS_420], "rot90"), lambda: V.swap_sbs_jpeg(files[SBS_444]))


def _report_cases(V, images):
    from vr180_convert_amd.jpeg_compose_device import last_compose_report
    from vr180_convert_amd.jpeg_transcode_device import last_transcode_report

    files = DC.supported_cases()
    return {
        "encode_batch": ("v1c_jpeg_encode_batch", lambda: V.encode_jpeg_tensors([images[k] for k in ("l0", "l1", "l2")]),
                         lambda: V.encode_jpeg_tensors([images[k] for k in ("m0", "m1")]), V.last_encode_batch_report),
        "decode": ("v1c_jpeg_decode", lambda: V.decode_jpeg_tensor(files[DECODE_0]).cpu().numpy().tobytes(),
                   lambda: V.decode_jpeg_tensor(files[DECODE_256]).cpu().numpy().tobytes(), V.last_decode_report),
        "decode_batch": ("v1c_jpeg_decode_batch", lambda: [t.cpu().numpy().tobytes() for t in V.decode_jpeg_tensors([files[n] for n in DECODE_BATCH])],
                         lambda: [t.cpu().numpy().tobytes() for t in V.decode_jpeg_tensors([files[DECODE_0], files[DECODE_256]])], V.last_batch_report),
        "transcode": ("v1c_jpeg_transcode", lambda: V.split_sbs_jpeg(files[SBS_420]), lambda: V.swap_sbs_jpeg(files[SBS_444]), last_transcode_report),
        "compose": ("v1c_jpeg_compose", lambda: V.transform_jpeg(files[SBS_420], "rot90"), lambda: V.transform_jpeg(files[DECODE_0], "flip_v"),
                    last_compose_report),
    }


@pytest.mark.parametrize("kind", ["encode_batch", "decode", "decode_batch", "transcode", "compose"])
def test_reports_are_the_calling_threads(V, images, monkeypatch, kind):
    """B's call lies inside A's, and B makes it once more after A's has come back; then each thread asks for its last report and is told
    about its own call"""
    entry, call_a, call_b, report = _report_cases(V, images)[kind]
    want_a = call_a(), report()
    want_b = call_b(), report()
    assert want_a[1] != want_b[1] and want_a[1] and want_b[1]
    got_a, got_b = interleave(monkeypatch, entry, call_a, call_b, report)
    assert got_a == want_a and got_b == want_b, (got_a[1], want_a[1], got_b[1], want_b[1])
    assert report() == want_b[1]  # (the test's thread: still its own last call)


# ---- (c) the Python layer under plain concurrency --------------------------------------------------------------------------------------
def test_python_layer_from_four_threads(V):
    """four threads behind a barrier, six rounds: each encodes an image of its own to JPEG and to PNG, decodes a file of its own and
    splits one, and gets what the same calls give serially.  The soak half of the fixed interleavings above: it may pass by luck."""
    from vr180_convert_amd import png_device as P

    rounds = 6
    decode = [DC.supported_cases()[n] for n in (DECODE_256, DECODE_0, "size_17x17_420", "noise_q100_gray")]
    split = [XC.cases()[f"optimize_noise_{kind}"][0] for kind in XC.KINDS]
    imgs = [torch.from_numpy(A.noise(np.uint8, 48 + 16 * k, 64 + 8 * k, 3, 100 + k)).cuda() for k in range(THREADS)]

    def calls(k):
        return {"encode_jpeg_tensor": lambda: V.encode_jpeg_tensor(imgs[k]), "encode_png_tensor": lambda: P.encode_png_tensor(imgs[k]),
                "decode_jpeg_tensor": lambda: V.decode_jpeg_tensor(decode[k]).cpu().numpy().tobytes(), "split_sbs_jpeg": lambda: V.split_sbs_jpeg(split[k])}

    want = [{name: call() for name, call in calls(k).items()} for k in range(THREADS)]
    assert len({w["encode_jpeg_tensor"] for w in want}) == THREADS and len({w["split_sbs_jpeg"] for w in want}) == THREADS
    barrier, stop, wrong = threading.Barrier(THREADS), threading.Event(), []

    def worker(k):
        def run(stream):
            try:
                for r in range(rounds):
                    barrier.wait(JOIN_TIMEOUT)
                    for name, call in calls(k).items():
                        if stop.is_set():
                            return
                        if call() != want[k][name]:
                            wrong.append((k, r, name))
            except threading.BrokenBarrierError:  # (another thread raised)
                return
            except BaseException:
                stop.set()
                raise
            finally:
                if stop.is_set():
                    barrier.abort()
        return run

    run_threads({f"codec-{k}": worker(k) for k in range(THREADS)})
    assert not wrong, wrong[:8]
