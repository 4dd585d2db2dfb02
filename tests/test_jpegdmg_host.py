"""Damaged scans without a GPU (tests/jpgdmg_cases.py): the conditions that keep the two lists in the entropy decoder and out of the
parse; the restatements against their own plain decoders on every damaged file that is still a legal stream; the product's host
builds -- tests/host_jpegdec, tests/host_jpegdec_prog, tests/host_jpegdec_batch -- against the restatement in return code, error bit,
error scan, rounds and pixels with 0 differing, on the lists the GPU half runs and on a longer draw of the same generator; the lossless
entries' host builds (tests/host_jpegxc, tests/host_jpegxf) on a damaged source against jpgxc_ref / jpgxf_ref; and the cases of
the GPU fuzz slices (--jpegdmg, --jpegodd) through the host builds.  A disagreement between ``*_core.hpp`` and the contract shows here first;
tests/test_gpu_jpegdmg.py then holds the kernels to the same verdicts.  The stand-alone sanitizer runs of the five host tests take
the same files."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import jpgdmg_cases as M
import test_jpegdec_batch_host as TB
import test_jpegdec_host as TD
import test_jpegprog_host as TP

CODE = {"decoded": 0, "unsupported": 1, "parse": 2, "refused": 3}   # what the host builds return
LONGER = 128                                                         # files of the longer draw, per decoder
DECODERS = [pytest.param(False, id="sequential"), pytest.param(True, id="progressive")]


def _build(harness, out):
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-fno-fast-math", "-o", str(out),
                    str(harness)], check=True, capture_output=True, timeout=600)
    return C.CDLL(str(out))


@pytest.fixture(scope="module")
def emul_seq(tmp_path_factory):
    lib = _build(TD.HARNESS, tmp_path_factory.mktemp("dmg_jpegdec") / "libjpegdec_emul.so")
    vp, u32 = C.c_void_p, C.c_uint32
    lib.jdec_emul_info.argtypes = [C.c_char_p, C.c_uint64, vp]
    lib.jdec_emul_decode.argtypes = [C.c_char_p, C.c_uint64, u32, C.c_int, vp, vp, vp, u32, vp, vp]
    return lib


@pytest.fixture(scope="module")
def emul_prog(tmp_path_factory):
    lib = _build(TP.HARNESS, tmp_path_factory.mktemp("dmg_jpegprog") / "libjpegprog_emul.so")
    vp, u32 = C.c_void_p, C.c_uint32
    lib.jprog_emul_info.argtypes = [C.c_char_p, C.c_uint64, vp]
    lib.jprog_emul_decode.argtypes = [C.c_char_p, C.c_uint64, u32, C.c_int, vp, u32, vp, vp, u32, vp, vp, vp, vp]
    return lib


@pytest.fixture(scope="module")
def emul_batch(tmp_path_factory):
    return TB._build(tmp_path_factory.mktemp("dmg_jpegdec_batch") / "libjpegdec_batch_emul.so")


# ---- the lists ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prog", DECODERS)
def test_the_lists_stay_in_the_entropy_decoder(prog):
    """per decoder and subsequence size: at least a third of the files refused by the last pass, at least an eighth decoded, at most a
    quarter left to the parse; every kind refused by the last pass at least once, every random kind decoded at least once.  By the
    restatement alone.  The counts are printed: the module's docstring and INTEGRATION.md quote them."""
    cases = M.cases(prog)
    src = M.sources(prog)
    n = len(cases)
    assert 64 <= n <= M.LIMIT
    for S in M.SUBSEQ:
        sh = M.shares(prog, S)
        refused, decoded, parse = (sum(v[i] for v in sh.values()) for i in range(3))
        unsup = sum(M.verdict(x.name, S, prog).what == "unsupported" for x in cases)
        print(f"{'progressive' if prog else 'sequential'} S={S}: {n} files, refused by the last pass {refused}, decoded {decoded}, "
              f"parse {parse} (of them unsupported {unsup});", ", ".join(f"{k} {v[0]}/{v[1]}/{v[2]}" for k, v in sh.items()))
        assert 3 * refused >= n and 8 * decoded >= n and 4 * parse <= n
        assert all(v[0] >= 1 for v in sh.values()), sh
        assert all(sh[k][1] >= 1 for k in M.RANDOM_KINDS), sh
        assert set(M.RANDOM_KINDS) < set(sh)
        # a refusal at bit 0 reports what a clean report holds: at least a third of the refusals name another bit
        bits = [M.verdict(x.name, S, prog).bit for x in cases if M.verdict(x.name, S, prog).what == "refused"]
        print(f"    refusals at a bit other than 0: {sum(b != 0 for b in bits)} of {len(bits)}")
        assert 3 * sum(b != 0 for b in bits) >= len(bits)
    # all three fills, whatever the seed; each reaches the last pass
    assert {x.name.split(":")[2] for x in cases if x.kind == "fill"} >= set(M.FILLS)
    assert all(M.verdict(x.name, 256, prog).what in ("refused", "decoded") for x in cases if x.kind == "fill")
    if not prog:
        for x in cases:
            if x.kind == "fill":
                a, e = M.scan_ranges(src[x.base], False)[0]
                body = x.data[a:a + (e - a)]
                if x.name.endswith(":zeros"):
                    assert not any(body), x.name
                if x.name.endswith(":ff00"):
                    assert body[:-1] == (b"\xff\x00" * len(body))[:len(body) - 1], x.name
        # the all-ones stream on a file whose last pass takes two workgroups of 256 subsequences: every lane of both reports
        v = M.verdict("noise_q100_444:fill:ff00", 256, False)
        assert (v.what, v.bit) == ("refused", 0) and v.subsequences > 256
        # two segments refused, the later one in the second workgroup, the earlier one's bit the verdict and not 0
        x = next(c for c in cases if c.name.endswith(":swap:short_last"))
        v, s = M.verdict(x.name, 256, False), M.D.parse(x.data)
        st = M.D.Stream(s, 256)
        assert v.what == "refused" and v.bit == 8 * s.segoff[1] > 0 and st.subfirst[1] < 256 <= st.subfirst[4] and s.nseg == 5
    # the damage lies where it is said to lie: a random kind leaves everything in front of the first scan alone, and every file of
    # the lists parses up to its first SOS as its base does
    for x in cases:
        if x.kind in M.RANDOM_KINDS:
            a = M.scan_ranges(src[x.base], prog)[0][0]
            assert x.data[:a] == src[x.base][:a] and x.data != src[x.base], x.name
    if prog:
        # for each of the four scan kinds, a file whose EARLIEST bad scan is of that kind; the run past its segment; the correction
        # bits; a scan behind a DRI change
        for kind, name in enumerate(M.SCAN_KINDS):
            hit = [x for x in cases if x.kind == name and M.verdict(x.name, 256, True).what == "refused"]
            assert hit and all(M.P.parse(x.data).scans[M.verdict(x.name, 256, True).scan].kind == kind for x in hit), name
        v = M.verdict("w_eobrun_40:eobrun:past_segment", 256, True)
        assert (v.what, v.scan, v.bit) == ("refused", 1, 0)
        # the correction bits: every byte that differs lies in the last scan behind its symbol and run length; flipped correction bits
        # are a legal stream with other pixels, a deleted byte leaves the run short of bits and is refused in that scan
        base = src["w_correction_run"]
        a, e = M.scan_ranges(base, True)[3]
        for x in cases:
            if x.kind == "correction":
                first = next(i for i, (p, q) in enumerate(zip(x.data, base)) if p != q)
                v = M.verdict(x.name, 256, True)
                assert a + M.CORRECTION_HEAD <= first < e and x.data[:a] == base[:a], x.name
                if len(x.data) == len(base):
                    assert v.what == "decoded" and not np.array_equal(v.pixels, M.verdict_of(base, 256, True).pixels), x.name
                else:
                    assert (v.what, v.scan) == ("refused", 3), x.name
        assert {M.verdict(x.name, 256, True).scan for x in cases if x.kind == "dri_changed"} >= {5, 6, 7}


@pytest.mark.parametrize("prog", DECODERS)
def test_restatement_against_its_plain_decoder(prog):
    """on every damaged file that decodes: the plain decoder's coefficients and states are the iteration's, rounds <= subsequences + 1
    (asserted in ``verdict_of``), and the pixels do not depend on the subsequence size"""
    n = 0
    for x in M.cases(prog):
        if M.verdict(x.name, 256, prog).what != "decoded":
            continue
        n += 1
        for S in M.SUBSEQ:
            v = M.verdict_of(x.data, S, prog, check=True)
            assert v.what == "decoded" and v.rounds == M.verdict(x.name, S, prog).rounds, x.name
            assert np.array_equal(v.pixels, M.verdict(x.name, 256, prog).pixels), x.name
    assert n >= M.LIMIT // 8


def test_the_verdict_does_not_depend_on_the_subsequence_size():
    for prog in (False, True):
        for x in M.cases(prog):
            a, b = (M.verdict(x.name, S, prog) for S in M.SUBSEQ)
            assert (a.what, a.bit, a.scan) == (b.what, b.bit, b.scan), x.name


# ---- the host builds ------------------------------------------------------------------------------------------------------------------
def seq_differences(lib, data, S, want):
    """what of the sequential host build's answer is not the restatement's"""
    rc, info = TD._emul_info(lib, data)
    if rc != 0 or want.what in ("unsupported", "parse"):
        return [] if rc == CODE[want.what] else [f"parse rc {rc}"]
    rc, coef, states, counts, report, px = TD._emul_decode(lib, data, S)
    bad = []
    if rc != CODE[want.what]:
        bad.append(f"rc {rc}")
    if report[:3].tolist() != [want.segments, want.subsequences, want.rounds]:
        bad.append(f"report {report[:3].tolist()} for {[want.segments, want.subsequences, want.rounds]}")
    if want.what == "refused" and int(report[3]) != want.bit:
        bad.append(f"bit {int(report[3])} for {want.bit}")
    if want.what == "decoded" and not np.array_equal(px, want.pixels):
        bad.append(f"{int((px != want.pixels).sum())} differing bytes")
    return bad


def prog_differences(lib, data, S, want):
    rc, info = TP._emul_info(lib, data)
    if rc != 0 or want.what in ("unsupported", "parse"):
        return [] if rc == CODE[want.what] else [f"parse rc {rc}"]
    rc, after, states, counts, rounds, nsub, report, px = TP._emul_decode(lib, data, S)
    bad = []
    if rc != CODE[want.what]:
        bad.append(f"rc {rc}")
    if int(report[2]) != want.rounds:
        bad.append(f"rounds {int(report[2])} for {want.rounds}")
    if want.what == "refused" and (int(report[3]), int(report[4])) != (want.bit, want.scan):
        bad.append(f"bit {int(report[3])} of scan {int(report[4])} for bit {want.bit} of scan {want.scan}")
    if want.what == "decoded":
        if list(rounds) != want.scan_rounds or int(report[1]) != want.subsequences:
            bad.append(f"rounds per scan {list(rounds)} for {want.scan_rounds}")
        if not np.array_equal(px, want.pixels):
            bad.append(f"{int((px != want.pixels).sum())} differing bytes")
    return bad


@pytest.mark.parametrize("prog", DECODERS)
def test_host_build_equals_restatement_on_the_lists(emul_seq, emul_prog, prog):
    """return code, error bit, error scan, rounds (per scan) and pixels at both sizes: 0 differing"""
    lib, diff = (emul_prog, prog_differences) if prog else (emul_seq, seq_differences)
    bad = {(x.name, S): d for x in M.cases(prog) for S in M.SUBSEQ if (d := diff(lib, x.data, S, M.verdict(x.name, S, prog)))}
    assert not bad, bad


@pytest.mark.parametrize("prog", DECODERS)
def test_host_build_equals_restatement_on_a_longer_draw(emul_seq, emul_prog, prog):
    """further files of the same generator, at alternating subsequence sizes"""
    lib, diff = (emul_prog, prog_differences) if prog else (emul_seq, seq_differences)
    bad, seen = {}, {}
    for k, x in enumerate(M.longer_draw(prog, LONGER)):
        S = M.SUBSEQ[k & 1]
        want = M.verdict_of(x.data, S, prog)
        seen[want.what] = seen.get(want.what, 0) + 1
        d = diff(lib, x.data, S, want)
        if d:
            bad[(x.name, S)] = d
    print("longer draw:", seen)
    assert not bad, bad
    assert seen["refused"] >= LONGER // 4 and seen["decoded"] >= LONGER // 8


# ---- the batch ------------------------------------------------------------------------------------------------------------------------
def chunk_budget(ws, live, damaged):
    """the smallest budget under which, among the files the parse accepts (``live``), a damaged file opens a chunk and another closes
    one, with three to five chunks; ``ws``: every live file's workspace"""
    sums = sorted({sum(ws[i:j]) for i in range(len(ws)) for j in range(i + 1, len(ws) + 1)})
    for b in sums:
        ends = M.chunk_ends(ws, b)
        starts = [0] + ends[:-1]
        if 3 <= len(ends) <= 5 and any(live[s] in damaged for s in starts[1:]) and any(live[e - 1] in damaged for e in ends[:-1]):
            return b, ends
    raise AssertionError("no such budget")


@pytest.mark.parametrize("S", M.SUBSEQ)
@pytest.mark.parametrize("name", ["mixed", "all_damaged", "chunked"])
def test_batch_host_build_gives_every_file_the_single_calls_answer(emul_batch, name, S):
    """the three batches of ``jpgdmg_cases.batches``: every file's status, bit and rounds are the restatement's for the file alone,
    every file that decodes is exact, and the batch's rounds are the sum over the chunks of their slowest file's"""
    files = M.batches()[name]
    wants = M.batch_wants(files, S)
    data = [d for _, _, d in files]
    live = [i for i, w in enumerate(wants) if w.what in ("decoded", "refused")]
    budget, ends = 0, [len(live)]
    if name == "chunked":
        ws = [emul_batch.jdecb_workspace(data[i], len(data[i]), S) for i in live]
        budget, ends = chunk_budget(ws, live, {i for i, f in enumerate(files) if f[0] and wants[i].what == "refused"})
        # (what the GPU half passes as max_workspace_bytes, and the chunks it must then report)
        assert (budget, [live[e - 1] + 1 for e in ends]) == (M.CHUNK_BUDGET[S], M.CHUNK_ENDS[S])
    res, (rounds, chunks) = TB.run_batch(emul_batch, data, S, budget)
    for i, (r, w) in enumerate(zip(res, wants)):
        assert r.status == CODE[w.what], (name, i, files[i][0] or files[i][1])
        if w.what in ("decoded", "refused"):
            assert r.report[:3] == [w.segments, w.subsequences, w.rounds], (name, i)
        if w.what == "refused":
            assert r.report[3] == w.bit, (name, i)
        if w.what == "decoded":
            assert np.array_equal(r.pixels, w.pixels), (name, i)
    assert chunks == len(ends) and rounds == M.batch_rounds_of([wants[i] for i in live], ends)
    if name == "mixed":
        assert files[0][0] is not None and files[-1][0] is not None and wants[0].what == wants[-1].what == "refused"
    if name == "all_damaged":
        assert all(f[0] for f in files) and {CODE[w.what] for w in wants} >= {0, 3} and {CODE[w.what] for w in wants} & {1, 2}


# ---- the lossless entries -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul_xf(tmp_path_factory):
    """(tests/host_jpegxf includes tests/host_jpegxc: one build has both)"""
    import test_jpegxf_host as TF

    lib = _build(TF.HARNESS, tmp_path_factory.mktemp("dmg_jpegxf") / "libjpegxf_emul.so")
    lib.jxc_emul_transcode.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.jxf_emul_compose.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
                                     C.c_void_p]
    lib.jxc_emul_error_bit.restype = C.c_uint32
    return lib


@pytest.mark.parametrize("S", M.SUBSEQ)
def test_lossless_host_builds_on_a_damaged_source(emul_xf, S):
    """every file of the sequential list as the source of a whole-image transcode and as the second source of a join behind its sound
    base: the restatement's code; where the last pass refuses, the damaged source is source 1 and the bit is the decoder's; where the
    source decodes, the restatement's bytes or its out-of-range refusal"""
    import test_jpegxc_host as TX
    import test_jpegxf_host as TF

    seen = {}
    for x in M.sequential_cases():
        v = M.verdict(x.name, S, False)
        out, code, want = M.transcode_want(x.name)
        rc, made = TX.run_emul(emul_xf, x.data, [out], S, M.shape_of(x))
        assert rc == code and (code != 0 or made[0][1] == want), (x.name, rc, code)
        if v.what == "refused":
            assert emul_xf.jxc_emul_error_bit() == v.bit, x.name
        seen[("transcode", code)] = seen.get(("transcode", code), 0) + 1
        j = M.join_want(x.name)
        if j is None:
            continue
        out, code, want = j
        rc, made, damaged = TF.run_emul(emul_xf, [M.base_of(x), x.data], [out], S)
        assert rc == code and (code != 0 or made[0][1] == want), (x.name, rc, code)
        if v.what == "refused":
            assert damaged == 1 and emul_xf.jxc_emul_error_bit() == v.bit, x.name
        seen[("join", code)] = seen.get(("join", code), 0) + 1
    print(seen)
    assert seen[("transcode", 0)] >= 12 and seen[("join", 0)] >= 12 and seen[("transcode", -5)] >= 32 and seen[("join", -5)] >= 32


# ---- the fuzz slice -------------------------------------------------------------------------------------------------------------------
def fuzz_module():
    import importlib.util
    import sys
    from pathlib import Path

    if "v1c_tools_fuzz" not in sys.modules:
        spec = importlib.util.spec_from_file_location("v1c_tools_fuzz", Path(__file__).resolve().parents[1] / "tools" / "fuzz.py")
        sys.modules["v1c_tools_fuzz"] = mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    return sys.modules["v1c_tools_fuzz"]


def test_the_fuzz_slices_cases_on_the_host_builds(emul_seq, emul_prog, product_lib):
    """the 40 cases tests/test_gpu_fuzz_jpegdmg.py sends to the device, drawn here as tools/fuzz.py draws them under the same seed:
    the host builds give the restatement's verdict on every one, and the restatement alone refuses at least 10 in the last pass and
    decodes at least 5"""
    F = fuzz_module()
    seen, bad = {}, {}
    for case in range(M.FUZZ_CASES):
        rng = np.random.default_rng([M.FUZZ_SEED, case])
        rng.random()                                          # (the tool draws the case's share first)
        desc, data, prog, S = F.jpegdmg_draw(rng)
        want = M.verdict_of(data, S, prog)
        seen[want.what] = seen.get(want.what, 0) + 1
        d = (prog_differences(emul_prog, data, S, want) if prog else seq_differences(emul_seq, data, S, want))
        if d:
            bad[case] = (desc, d)
    print("fuzz slice:", seen)
    assert not bad, bad
    assert seen.get("refused", 0) >= 10 and seen.get("decoded", 0) >= 5
    # the cases of the --jpegodd slice (tests/test_gpu_fuzz_jpegodd.py): legal files of unusual structure and damaged headers
    import jpgodd_cases as O

    seen, kinds = {}, {}
    for case in range(O.FUZZ_CASES):
        rng = np.random.default_rng([O.FUZZ_SEED, case])
        rng.random()
        desc, data, prog, S = F.jpegodd_draw(rng)
        v = O.header_verdict_of(data, S, prog)
        kinds[" odd legal " in desc] = kinds.get(" odd legal " in desc, 0) + 1
        seen[v.what] = seen.get(v.what, 0) + 1
        rc, _ = (TP if prog else TD)._emul_info(emul_prog if prog else emul_seq, data)
        if rc != {"parsed": 0, "unsupported": 1, "corrupt": 2}[v.what]:
            bad[case] = (desc, f"parse rc {rc} for {v.what}")
        elif v.inner is not None:
            d = (prog_differences(emul_prog, data, S, v.inner) if prog else seq_differences(emul_seq, data, S, v.inner))
            if d:
                bad[case] = (desc, d)
    print("jpegodd slice:", seen, kinds)
    assert not bad, bad
    assert kinds.get(True, 0) >= 10 and kinds.get(False, 0) >= 10 and seen.get("corrupt", 0) >= 5
