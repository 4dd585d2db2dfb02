"""Damaged scans on the MI355X: the two lists of tests/jpgdmg_cases.py -- exactly the files whose host-build and stand-alone sanitizer
runs tests/test_jpegdmg_host.py and the decoders' host tests hold -- through ``v1c_jpeg_decode``, ``v1c_jpeg_prog_decode``, the Python
layer, ``v1c_jpeg_decode_batch``, ``v1c_jpeg_transcode`` and ``v1c_jpeg_compose`` at 256- and 1024-bit subsequences.  Every number
compared is the restatement's (``jpgdmg_cases.verdict``): the return code, the smallest bad bit (of the earliest bad scan), the rounds
also of a refused file, and the pixels of damage that is still a legal stream, with 0 differing bytes.  What the host builds do not
share is what this file is for: the kernels' decomposition, the two exit buffers, the flag words, the error word taken across
workgroups, the per-file flags of a batch, the per-scan verdict of a progressive file, and what a refused call leaves behind."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpgdmg_cases as M

pytestmark = pytest.mark.gpu
OK, UNSUPPORTED, CORRUPT = 0, -2, -5
CODE = {"decoded": OK, "unsupported": UNSUPPORTED, "parse": CORRUPT, "refused": CORRUPT}
GUARD = 0x5A


class Report(C.Structure):
    _fields_ = [("segments", C.c_uint32), ("subsequences", C.c_uint32), ("rounds", C.c_uint32), ("reserved", C.c_uint32),
                ("error_pos", C.c_uint64)]


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


# ---- outputs with a guard band --------------------------------------------------------------------------------------------------------
class Guarded:
    """an (h, w, 3) device tensor inside a larger one filled with 0x5A: rows pitched by 13 bytes more than they hold, a tail of 64"""

    def __init__(self, h, w):
        self.h, self.w, self.pitch = h, w, 3 * w + 13
        self.whole = torch.full((h * self.pitch + 64,), GUARD, dtype=torch.uint8, device="cuda")
        self.view = self.whole[:h * self.pitch].view(h, self.pitch)[:, :3 * w].unflatten(1, (w, 3))

    def pixels(self):
        return self.whole.cpu().numpy()[:self.h * self.pitch].reshape(self.h, self.pitch)[:, :3 * self.w].reshape(self.h, self.w, 3)

    def band_untouched(self):
        got = self.whole.cpu().numpy()
        rows = got[:self.h * self.pitch].reshape(self.h, self.pitch)
        return bool((rows[:, 3 * self.w:] == GUARD).all() and (got[self.h * self.pitch:] == GUARD).all())


def size_of(x, prog):
    """(h, w) of the output a caller would allocate: the file's own where the parse takes it, else its base's"""
    for data in (x.data, M.sources(prog)[x.base]):
        try:
            s = (M.P.parse if prog else M.D.parse)(data)
            return s.h, s.w
        except (M.D.Corrupt, M.D.Unsupported):
            continue
    return 8, 8


def seq_decode(lib, data, S, out):
    rep = Report()
    rc = lib.v1c_jpeg_decode(0, torch.cuda.current_stream().cuda_stream, data, len(data), out.data_ptr(), out.stride(0), 3, S, C.byref(rep))
    return rc, rep


def prog_decode(lib, data, S, out, scans):
    from vr180_convert_amd import _abi

    rep = _abi.JpegProgReport()
    per = (C.c_uint32 * max(scans, 1))()
    rc = lib.v1c_jpeg_prog_decode(0, torch.cuda.current_stream().cuda_stream, data, len(data), out.data_ptr(), out.stride(0), 3, S, C.byref(rep),
                                  per, scans)
    return rc, rep, list(per)[:scans]


# ---- the two decoders through the C ABI -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", M.SUBSEQ)
def test_sequential_decoder_gives_the_restatements_verdict(lib, S):
    """every file of the list: code, bit, rounds (of refused files too), segments, subsequences, and the pixels of what decodes; the
    guard band untouched after every call; a sound decode behind every tenth damaged one, on the same stream with no device-wide
    synchronisation in between, byte-exact"""
    sound = M.DC.supported_cases()["midrow_420_r3"]
    sound_want = M.verdict_of(sound, S, False)
    bad = {}
    for k, x in enumerate(M.sequential_cases()):
        want = M.verdict(x.name, S, False)
        g = Guarded(*size_of(x, False))
        rc, rep = seq_decode(lib, x.data, S, g.view)
        msg = lib.v1c_last_error().decode()
        assert rc in (OK, UNSUPPORTED, CORRUPT), (x.name, rc, msg)      # (a HIP failure: nothing more goes to the device)
        if k % 10 == 9:                                    # (before anything of the damaged call is read back)
            h = Guarded(*sound_want.pixels.shape[:2])
            rc2, rep2 = seq_decode(lib, sound, S, h.view)
            assert rc2 == OK, (x.name, rc2, lib.v1c_last_error())
        d = []
        if rc != CODE[want.what]:
            d.append(f"rc {rc} for {CODE[want.what]}")
        if want.what in ("decoded", "refused") and (rep.segments, rep.subsequences, rep.rounds) != (want.segments, want.subsequences, want.rounds):
            d.append(f"report {(rep.segments, rep.subsequences, rep.rounds)} for {(want.segments, want.subsequences, want.rounds)}")
        if want.what == "refused" and (rep.error_pos != want.bit or f"bit {want.bit} " not in msg):
            d.append(f"bit {rep.error_pos} for {want.bit}")
        if want.what == "decoded" and not np.array_equal(g.pixels(), want.pixels):
            d.append(f"{int((g.pixels() != want.pixels).sum())} differing bytes")
        if not g.band_untouched():
            d.append("guard band written")
        if k % 10 == 9:
            if rc2 != OK or rep2.rounds != sound_want.rounds or not np.array_equal(h.pixels(), sound_want.pixels) or not h.band_untouched():
                d.append("the sound decode behind it is not exact")
        if d:
            bad[x.name] = d
        print(x.name, S, want.what, want.bit, want.rounds, "device:", rc, int(rep.error_pos), rep.rounds, d)
    assert not bad, bad


@pytest.mark.parametrize("S", M.SUBSEQ)
def test_progressive_decoder_gives_the_restatements_verdict(lib, S):
    """as above, with the earliest bad scan and the rounds per scan: of every scan where the file decodes, up to and including the
    refused scan where it does not"""
    sound = M.PCS.supported_cases()["w_dri_changed_420"]
    sound_want = M.verdict_of(sound, S, True)
    bad = {}
    for k, x in enumerate(M.progressive_cases()):
        want = M.verdict(x.name, S, True)
        g = Guarded(*size_of(x, True))
        scans = len(M.P.parse(x.data).scans) if want.what in ("decoded", "refused") else 0
        rc, rep, per = prog_decode(lib, x.data, S, g.view, scans)
        msg = lib.v1c_last_error().decode()
        assert rc in (OK, UNSUPPORTED, CORRUPT), (x.name, rc, msg)      # (a HIP failure: nothing more goes to the device)
        if k % 10 == 9:                                    # (before anything of the damaged call is read back)
            h = Guarded(*sound_want.pixels.shape[:2])
            rc2, rep2, per2 = prog_decode(lib, sound, S, h.view, len(sound_want.scan_rounds))
            assert rc2 == OK, (x.name, rc2, lib.v1c_last_error())
        d = []
        if rc != CODE[want.what]:
            d.append(f"rc {rc} for {CODE[want.what]}")
        if want.what in ("decoded", "refused") and rep.rounds != want.rounds:
            d.append(f"rounds {rep.rounds} for {want.rounds}")
        if want.what == "refused":
            if (rep.error_pos, rep.error_scan) != (want.bit, want.scan) or f"bit {want.bit} of unstuffed scan {want.scan}" not in msg:
                d.append(f"bit {rep.error_pos} of scan {rep.error_scan} for bit {want.bit} of scan {want.scan}")
            if per[:want.scan + 1] != want.scan_rounds:
                d.append(f"rounds per scan {per[:want.scan + 1]} for {want.scan_rounds}")
        if want.what == "decoded":
            if per != want.scan_rounds or (rep.scans, rep.segments, rep.subsequences) != (scans, want.segments, want.subsequences):
                d.append(f"rounds per scan {per} for {want.scan_rounds}, report {(rep.scans, rep.segments, rep.subsequences)}")
            if not np.array_equal(g.pixels(), want.pixels):
                d.append(f"{int((g.pixels() != want.pixels).sum())} differing bytes")
        if not g.band_untouched():
            d.append("guard band written")
        if k % 10 == 9:
            if rc2 != OK or per2 != sound_want.scan_rounds or not np.array_equal(h.pixels(), sound_want.pixels) or not h.band_untouched():
                d.append("the sound decode behind it is not exact")
        if d:
            bad[x.name] = d
        print(x.name, S, want.what, want.bit, want.scan, want.rounds, "device:", rc, int(rep.error_pos), rep.error_scan, rep.rounds, d)
    assert not bad, bad


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", M.SUBSEQ)
@pytest.mark.parametrize("prog", [False, True], ids=["sequential", "progressive"])
def test_python_layer_names_the_same_bit(V, prog, S):
    """``decode_jpeg_tensor`` raises CorruptJPEG naming the restatement's bit (and scan), NotImplementedError for what the parse calls
    unsupported, and returns the restatement's pixels for what decodes; ``last_decode_report()`` is that of the last call that decoded,
    whatever was refused since"""
    from vr180_convert_amd import jpeg_decode_device as J

    last = None
    for x in M.cases(prog):
        want = M.verdict(x.name, S, prog)
        if want.what == "decoded":
            got = J.decode_jpeg_tensor(x.data, subseq_bits=S, progressive=prog).cpu().numpy()
            assert np.array_equal(got, want.pixels), x.name
            last = J.last_decode_report()
            assert (last["segments"], last["subsequences"], last["rounds"], last["path"]) == (want.segments, want.subsequences, want.rounds, "device")
            assert not prog or last["scan_rounds"] == want.scan_rounds, x.name
            continue
        with pytest.raises(NotImplementedError if want.what == "unsupported" else J.CorruptJPEG) as e:
            J.decode_jpeg_tensor(x.data, subseq_bits=S, progressive=prog)
        if want.what == "refused":
            assert f"bit {want.bit} of " + (f"unstuffed scan {want.scan}" if prog else "the unstuffed scan") in str(e.value), (x.name, str(e.value))
        elif want.what == "parse" and not prog:
            assert "byte" in str(e.value), x.name
        assert last is None or J.last_decode_report() == last, x.name


# ---- the batch ------------------------------------------------------------------------------------------------------------------------
def run_batch(lib, files, S, budget):
    """through the C ABI into guarded outputs: (status, reports, batch_rounds, outputs)"""
    n = len(files)
    outs = []
    for data in files:
        try:
            s = M.D.parse(data)
            outs.append(Guarded(s.h, s.w))
        except (M.D.Corrupt, M.D.Unsupported):
            outs.append(Guarded(8, 8))
    data_p = (C.c_char_p * n)(*files)
    sizes = (C.c_uint64 * n)(*[len(d) for d in files])
    ptrs = (C.c_void_p * n)(*[g.view.data_ptr() for g in outs])
    pitches = (C.c_int64 * n)(*[g.pitch for g in outs])
    cns = (C.c_int * n)(*([3] * n))
    status, reps, rounds = (C.c_int * n)(), (Report * n)(), C.c_uint32(0)
    rc = lib.v1c_jpeg_decode_batch(0, torch.cuda.current_stream().cuda_stream, n, data_p, sizes, ptrs, pitches, cns, S, budget, status, reps,
                                   C.byref(rounds))
    assert rc == OK, lib.v1c_last_error()
    return list(status), list(reps), int(rounds.value), outs


@pytest.mark.parametrize("S", M.SUBSEQ)
@pytest.mark.parametrize("name", ["mixed", "all_damaged", "chunked"])
def test_batch_gives_every_file_the_single_calls_answer(lib, name, S):
    """damaged files first, in the middle and last among sound ones; all files damaged; a budget under which a damaged file opens a
    chunk and another closes one: every file's status, error position and rounds are the restatement's for the file alone, every file
    that decodes is exact, and ``batch_rounds`` is what the per-file rounds imply"""
    files = M.batches()[name]
    wants = M.batch_wants(files, S)
    status, reps, rounds, outs = run_batch(lib, [d for _, _, d in files], S, M.CHUNK_BUDGET[S] if name == "chunked" else 0)
    for i, (w, st, rep, g) in enumerate(zip(wants, status, reps, outs)):
        assert st == CODE[w.what], (name, i, st)
        if w.what in ("decoded", "refused"):
            assert (rep.segments, rep.subsequences, rep.rounds) == (w.segments, w.subsequences, w.rounds), (name, i)
        if w.what == "refused":
            assert rep.error_pos == w.bit, (name, i, rep.error_pos, w.bit)
        if w.what == "decoded":
            assert np.array_equal(g.pixels(), w.pixels), (name, i, int((g.pixels() != w.pixels).sum()))
        assert g.band_untouched(), (name, i)
    # the chunks: where the host half found them to end under this budget, by the product's layout on the host
    live = [i for i, w in enumerate(wants) if w.what in ("decoded", "refused")]
    file_ends = M.CHUNK_ENDS[S] if name == "chunked" else [len(files)]
    assert [reps[i].reserved for i in live] == [sum(e <= i for e in file_ends) for i in live]    # (reserved: the file's chunk)
    ends = [sum(i < e for i in live) for e in file_ends]
    assert rounds == M.batch_rounds_of([wants[i] for i in live], ends)
    if name == "chunked":
        refused = {i for i, f in enumerate(files) if f[0] and wants[i].what == "refused"}
        assert any(e in refused for e in file_ends[:-1]) and any(e - 1 in refused for e in file_ends[:-1])


@pytest.mark.parametrize("S", M.SUBSEQ)
def test_python_batch_names_every_files_bit(V, S):
    from vr180_convert_amd import jpeg_decode_device as J

    files = M.batches()["mixed"]
    wants = M.batch_wants(files, S)
    got = V.decode_jpeg_tensors([d for _, _, d in files], subseq_bits=S, errors="return")
    rep = V.last_batch_report()
    for i, (w, t) in enumerate(zip(wants, got)):
        if w.what == "decoded":
            assert np.array_equal(t.cpu().numpy(), w.pixels), i
            assert rep["files"][i] == dict(segments=w.segments, subsequences=w.subsequences, rounds=w.rounds, path="device"), i
        elif w.what == "refused":
            assert isinstance(t, J.CorruptJPEG) and f"bit {w.bit} of the unstuffed scan" in str(t) and rep["files"][i] is None, (i, str(t))
        else:
            assert isinstance(t, NotImplementedError if w.what == "unsupported" else J.CorruptJPEG), i
    assert rep["batch_rounds"] == max(w.rounds for w in wants if w.rounds is not None) and rep["chunks"] == 1


# ---- the lossless entries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", M.SUBSEQ)
def test_transcode_and_compose_of_a_damaged_source(lib, S):
    """19 files of the sequential list as the source of a whole-image transcode and as the second source of a join behind their sound
    base: the code; the damaged source's report holds the restatement's bit and rounds, the other source's is clean; a damaged source
    that decodes gives the restatement's file byte for byte; and the sound transcode and the sound join behind every refusal are exact"""
    import jpgxc_ref as X
    import jpgxf_ref as F
    from test_gpu_jpegxc_edges import transcode
    from test_gpu_jpegxf import compose

    sound = {}
    for x in M.lossless_subset():
        v = M.verdict(x.name, S, False)
        base = M.base_of(x)
        if x.base not in sound:
            src = X.Source(base)
            pair = F.join_output(src, src, trim=True)
            sound[x.base] = (X.crop_output(src), X.transcode_jpeg(base), M.verdict_of(base, S, False).rounds, pair, F.compose([src, src], [pair])[0])
        out, code, want = M.transcode_want(x.name)
        rc, rep, files = transcode(lib, x.data, [out], S)
        assert rc == code and (code != OK or files == [want]), (x.name, rc, code, lib.v1c_last_error())
        if v.what == "refused":
            assert rep.error_pos == v.bit and rep.rounds == v.rounds and f"bit {v.bit} ".encode() in lib.v1c_last_error(), (x.name, rep.error_pos)
        if v.what == "decoded":
            assert rep.error_pos == 0 and rep.rounds == v.rounds, x.name
        j = M.join_want(x.name)
        if j is not None:
            out, code, want = j
            rc, reps, files, _ = compose(lib, [base, x.data], [out], S)
            assert rc in (OK, UNSUPPORTED, CORRUPT), (x.name, rc, lib.v1c_last_error())
            assert rc == code and (code != OK or files == [want]), (x.name, rc, code, lib.v1c_last_error())
            if v.what == "refused":
                assert reps[1].error_pos == v.bit and reps[1].rounds == v.rounds and reps[0].error_pos == 0, (x.name, reps[1].error_pos)
                assert f"of source 1 is damaged at bit {v.bit} ".encode() in lib.v1c_last_error(), x.name
            if v.what in ("decoded", "refused"):
                assert reps[0].rounds == sound[x.base][2], x.name
        if code != OK:
            out, want, rounds, pair, joined = sound[x.base]
            rc, rep, files = transcode(lib, base, [out], S)
            assert rc == OK and files == [want] and rep.rounds == rounds and rep.error_pos == 0, x.name
            rc, reps, files, _ = compose(lib, [base, base], [pair], S)
            assert rc == OK and files == [joined] and [r.rounds for r in reps] == [rounds, rounds] and not any(r.error_pos for r in reps), x.name
