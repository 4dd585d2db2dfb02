"""Odd legal files and damaged headers on the MI355X: the lists of tests/jpgodd_cases.py -- exactly the files that
tests/test_jpegodd_host.py holds on the host builds and sends through the stand-alone sanitizer programs -- through
``decode_jpeg_tensor`` (sequential and progressive), ``decode_jpeg_tensors``, ``transcode_jpeg`` and ``compose_regions``.  Every value
compared is a restatement's: pixels and files byte for byte, segments, subsequences and rounds of the reports, the bit a refusal names,
the byte a parse stops at.  What the host builds do not share is what this file is for: the kernels' lookup against their long path on
tables of drawn shape, the table selectors of drawn slots, rounds shared by files of different tables in one batch."""
import numpy as np
import pytest
import torch

import jpgdec_ref as D
import jpgodd_cases as O
import jpgxf_ref as F

pytestmark = pytest.mark.gpu
LEGAL = O.legal()
SEQ = [x for x in LEGAL if not x.prog]
PROG = [x for x in LEGAL if x.prog]
DEFAULT = D.DEFAULT_SUBSEQ_BITS


@pytest.fixture(scope="module")
def J():
    from vr180_convert_amd import jpeg_decode_device as J

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    return J


def _decode_one(J, data, prog, S, want, last, name):
    """one file through decode_jpeg_tensor against a jpgdmg_cases.Verdict; ``last``: the thread's report before the call, which a
    refusal must leave alone; returns the report behind the call"""
    kw = dict(progressive=prog) if S is None else dict(progressive=prog, subseq_bits=S)
    if want.what == "decoded":
        got = J.decode_jpeg_tensor(data, **kw).cpu().numpy()
        assert np.array_equal(got, want.pixels), (name, int((got != want.pixels).sum()))
        last = J.last_decode_report()
        assert (last["segments"], last["subsequences"], last["rounds"], last["path"]) == (want.segments, want.subsequences, want.rounds, "device"), name
        assert not prog or last["scan_rounds"] == want.scan_rounds, name
        return last
    with pytest.raises(NotImplementedError if want.what == "unsupported" else J.CorruptJPEG) as e:
        J.decode_jpeg_tensor(data, **kw)
    if want.what == "refused":
        assert f"bit {want.bit} of " + (f"unstuffed scan {want.scan}" if prog else "the unstuffed scan") in str(e.value), (name, str(e.value))
    assert J.last_decode_report() == last, name
    return last


# ---- the legal list -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [None, 256], ids=["default", "256"])
@pytest.mark.parametrize("sampling", O.SAMPLINGS)
def test_sequential_decoder_on_the_legal_list(J, sampling, S):
    """pixels and report at the default subsequence size and at 256 bits, the files of one sampling per case; a file of the group
    "complete" whose pad bits make up a block is refused at the restatement's bit"""
    last = J.last_decode_report()
    files = [x for x in SEQ if x.sampling == sampling]
    assert len(files) == len(SEQ) // 4
    for x in files:
        last = _decode_one(J, x.data, False, S, O.legal_verdict(x.name, S or DEFAULT), last, x.name)


@pytest.mark.parametrize("S", [None, 256], ids=["default", "256"])
@pytest.mark.parametrize("sampling", O.SAMPLINGS)
def test_progressive_decoder_on_the_legal_list(J, sampling, S):
    last = J.last_decode_report()
    files = [x for x in PROG if x.sampling == sampling]
    assert len(files) == len(PROG) // 4
    for x in files:
        last = _decode_one(J, x.data, True, S, O.legal_verdict(x.name, S or DEFAULT), last, x.name)


@pytest.mark.parametrize("S", [None, 256], ids=["default", "256"])
def test_batch_of_the_whole_legal_list(J, S):
    """every sequential file in one call: files of different table shapes and slots share the rounds"""
    wants = [O.legal_verdict(x.name, S or DEFAULT) for x in SEQ]
    got = J.decode_jpeg_tensors([x.data for x in SEQ], errors="return", **({} if S is None else dict(subseq_bits=S)))
    rep = J.last_batch_report()
    for i, (x, w, t) in enumerate(zip(SEQ, wants, got)):
        if w.what == "decoded":
            assert np.array_equal(t.cpu().numpy(), w.pixels), x.name
            assert rep["files"][i] == dict(segments=w.segments, subsequences=w.subsequences, rounds=w.rounds, path="device"), x.name
        else:
            assert isinstance(t, J.CorruptJPEG) and f"bit {w.bit} of the unstuffed scan" in str(t) and rep["files"][i] is None, (x.name, str(t))
    assert rep["batch_rounds"] == max(w.rounds for w in wants) and rep["chunks"] == 1


def _lossless(J, data, what, fallback, want_dec, name):
    """the whole image through transcode_jpeg and mirrored through compose_regions against the restatements' codes and bytes;
    returns the files the device made"""
    from vr180_convert_amd import jpeg_compose_device as JF
    from vr180_convert_amd import jpeg_transcode_device as JX

    made = {}
    out, code, want = O.transcode_want(data, what, fallback)
    flip = O.flip_want(data, what, fallback)
    calls = [("transcode", code, want, lambda: JX.transcode_jpeg(data))]
    if flip is not None:
        fo = dict(flip[0], regions=[(r[0], F.NAMES[r[1]]) + tuple(r[2:]) for r in flip[0]["regions"]])
        calls.append(("flip_h", flip[1], flip[2], lambda: JF.compose_regions([data], [fo])[0]))
    for which, code, want, call in calls:
        if code == 0:
            got = call()
            assert got == want, (name, which)
            rep = JX.last_transcode_report() if which == "transcode" else JF.last_compose_report()["sources"][0]
            assert (rep["segments"], rep["subsequences"], rep["rounds"]) == (want_dec.segments, want_dec.subsequences, want_dec.rounds), (name, which)
            made[which] = got
            continue
        with pytest.raises(NotImplementedError if code == -2 else J.CorruptJPEG) as e:
            call()
        if what == "refused":
            assert f"bit {want_dec.bit} " in str(e.value), (name, which, str(e.value))
    return made


@pytest.mark.parametrize("sampling", O.SAMPLINGS)
def test_lossless_entries_on_the_legal_list(J, sampling):
    """transcode_jpeg of the whole image and compose_regions under flip_h: the restatements' files byte for byte, the decode's report,
    and the file the DEVICE made, read back by the decoder's restatement, has the source's coefficients and quantisation tables"""
    done = 0
    for x in SEQ:
        if x.sampling != sampling:
            continue
        v = O.legal_verdict(x.name, DEFAULT)
        made = _lossless(J, x.data, v.what, None, v, x.name)
        done += len(made)
        assert ("transcode" in made) == (v.what == "decoded"), x.name
        if "transcode" in made:
            a, b = D.decode(x.data, check=False), D.decode(made["transcode"], check=False)
            assert np.array_equal(D.dc_values(a.info, a.coef), D.dc_values(b.info, b.coef)), x.name
            assert all(np.array_equal(a.info.q[a.info.tq[c]], b.info.q[b.info.tq[c]]) for c in range(a.info.nc)), x.name
    assert done >= 15


# ---- the damage lists -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", O.SUBSEQ)
@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("prog", [False, True], ids=["sequential", "progressive"])
def test_decoders_on_the_damage_lists(J, prog, kind, S):
    """a file the parse takes gives jpgdmg_cases' verdict: the pixels, or CorruptJPEG naming its bit; a corrupt header raises
    CorruptJPEG and an unsupported one NotImplementedError, both naming the byte the restatement's parse stops at, and the thread's
    last report stays what it was: the device was not reached"""
    last = J.last_decode_report()
    files = [x for x in O.header_damage(prog) if x.kind == kind]
    assert files
    for x in files:
        v = O.header_verdict(x.name, S, prog)
        if v.inner is not None:
            last = _decode_one(J, x.data, prog, S, v.inner, last, x.name)
            continue
        with pytest.raises(NotImplementedError if v.what == "unsupported" else J.CorruptJPEG) as e:
            J.decode_jpeg_tensor(x.data, subseq_bits=S, progressive=prog)
        assert f"(byte {v.pos})" in str(e.value), (x.name, x.how, str(e.value), v.why)
        assert J.last_decode_report() == last, x.name


def test_batch_on_the_sequential_damage_list(J):
    """the whole list in one call: every file the single call's answer"""
    cases = O.header_damage(False)
    got = J.decode_jpeg_tensors([x.data for x in cases], errors="return", subseq_bits=256)
    rep = J.last_batch_report()
    for i, (x, t) in enumerate(zip(cases, got)):
        v = O.header_verdict(x.name, 256, False)
        w = v.inner
        if w is not None and w.what == "decoded":
            assert np.array_equal(t.cpu().numpy(), w.pixels), x.name
            assert rep["files"][i] == dict(segments=w.segments, subsequences=w.subsequences, rounds=w.rounds, path="device"), x.name
        elif w is not None:
            assert isinstance(t, J.CorruptJPEG) and f"bit {w.bit} of the unstuffed scan" in str(t) and rep["files"][i] is None, (x.name, str(t))
        else:
            assert isinstance(t, NotImplementedError if v.what == "unsupported" else J.CorruptJPEG) and rep["files"][i] is None, (x.name, t)
            assert f"(byte {v.pos})" in str(t), (x.name, x.how, str(t))


@pytest.mark.parametrize("kind", O.KINDS)
def test_lossless_entries_on_the_sequential_damage_list(J, kind):
    from vr180_convert_amd import jpeg_compose_device as JF
    from vr180_convert_amd import jpeg_transcode_device as JX

    src = O.damage_sources(False)
    for x in O.header_damage(False):
        if x.kind != kind:
            continue
        v = O.header_verdict(x.name, DEFAULT, False)
        if v.inner is not None:
            made = _lossless(J, x.data, v.inner.what, src[x.base], v.inner, x.name)
            assert ("transcode" in made) == (O.transcode_want(x.data, v.inner.what, src[x.base])[1] == 0), x.name
            continue
        before = (JX.last_transcode_report(), JF.last_compose_report())
        for call in (lambda: JX.transcode_jpeg(x.data), lambda: JF.transform_jpeg(x.data, "flip_h", trim=True)):
            with pytest.raises(NotImplementedError if v.what == "unsupported" else J.CorruptJPEG) as e:
                call()
            assert f"(byte {v.pos})" in str(e.value), (x.name, str(e.value))
        assert (JX.last_transcode_report(), JF.last_compose_report()) == before, x.name
