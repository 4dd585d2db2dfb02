"""The batched device JPEG decoder without a GPU: the product's headers (jpegdec_core.hpp, jpegdec_host.hpp, jpegdec_batch.hpp and the
workspace layout of jpegdec_launch.hpp) in a sequential copy of the batched kernels' decomposition -- flat work lists, the per-workgroup
file lookup, rounds shared by the files with the rule that lets a converged file rest, per-file parity in the last pass, chunks under a
workspace budget -- against the restatement (jpgdec_ref.py) file by file; the same build broken on purpose three ways; the same build
as a stand-alone program under the address and undefined-behaviour sanitizers; the resource budget of the batched kernels; the Python
plumbing of ``decode_jpeg_tensors``, ``read_inputs(batch=True)`` and ``device_decode="batch"`` with the native call stubbed."""
import ctypes as C
import logging
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

import jpgdec_cases as DC
import jpgdmg_cases as M

ROOT = Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "host_jpegdec_batch" / "jpegdec_batch_emul.hip"
CASES = {**DC.supported_cases(), **DC.extreme_cases()}
SUBSEQ = (256, 1024, 4096)
NOISE = "noise_q100_420"        # 64 x 96, quality 100: the slowest to converge at 256 bits (232 rounds), two workgroups, the last partial
WIDE = "noise_q100_444"         # 64 x 96 as well: the most subsequences (785: four workgroups, the last partial), 154 rounds
SMOOTH = ("size_8x8_444", "flat_420", "size_17x17_420", "quality_1")


def _build(out, *flags):
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-fno-fast-math", *flags, "-o", str(out),
                    str(HARNESS)], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(out))
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.jdecb_info.argtypes = [C.c_char_p, u64, vp]
    lib.jdecb_workspace.argtypes = [C.c_char_p, u64, u32]
    lib.jdecb_workspace.restype = u64
    lib.jdecb_decode.argtypes = [C.c_int, vp, vp, u32, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    return lib


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("host_jpegdec_batch") / "libjpegdec_batch_emul.so")


class Result:
    pass


def run_batch(lib, files, S, budget=0):
    """the batch through the host build: per file a Result (status, report, error_pos, coef, states, counts, pixels), and (batch_rounds,
    chunks)"""
    n = len(files)
    res = []
    for data in files:
        r = Result()
        info = np.zeros(8, np.int32)
        ok = lib.jdecb_info(data, len(data), info.ctypes.data) == 0
        h, w, nblocks = (int(info[0]), int(info[1]), int(info[7])) if ok else (1, 1, 1)
        r.cap = len(data) * 8 // 256 + int(info[6]) + 1
        r.coef, r.states, r.counts = np.zeros((nblocks, 64), np.int16), np.zeros((r.cap, 3), np.uint32), np.zeros(r.cap, np.uint32)
        r.pixels = np.zeros((h, w, 3), np.uint8)
        res.append(r)
    ptrs = lambda arrs: (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    data_p = (C.c_char_p * n)(*files)
    sizes = np.array([len(d) for d in files], np.uint64)
    caps = np.array([r.cap for r in res], np.uint32)
    reports, error_pos, status, batch = np.zeros((n, 4), np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(2, np.uint32)
    rc = lib.jdecb_decode(n, data_p, sizes.ctypes.data, S, budget, ptrs([r.coef for r in res]), ptrs([r.states for r in res]),
                          ptrs([r.counts for r in res]), caps.ctypes.data, reports.ctypes.data, error_pos.ctypes.data,
                          ptrs([r.pixels for r in res]), status.ctypes.data, batch.ctypes.data)
    assert rc == 0
    for i, r in enumerate(res):
        r.status, r.report, r.error_pos = int(status[i]), reports[i].tolist(), int(error_pos[i])
        k = r.report[1]
        r.states, r.counts = r.states[:k], r.counts[:k]
    return res, (int(batch[0]), int(batch[1]))


def mismatches(res, names, S):
    """the files of a batch that are not the restatement's in report, coefficients, entry states, block counts or pixels"""
    bad = []
    for r, name in zip(res, names):
        want = DC.reference(name, S)
        ok = (r.status == 0 and r.report[:3] == [want.segments, want.subsequences, want.rounds] and np.array_equal(r.coef, want.coef)
              and [tuple(s) for s in r.states.tolist()] == want.entry and r.counts.tolist() == want.counts and np.array_equal(r.pixels, want.pixels))
        if not ok:
            bad.append(name)
    return bad


# ---- the batches --------------------------------------------------------------------------------------------------------------------
BATCHES = {
    "all": list(CASES),
    "reversed": list(CASES)[::-1],
    "one": ["size_17x17_420"],
    "two": [WIDE, "size_8x8_gray"],
    "spread": [SMOOTH[0], SMOOTH[1], NOISE, SMOOTH[2], WIDE, SMOOTH[3]],
}


@pytest.mark.parametrize("S", SUBSEQ)
@pytest.mark.parametrize("batch", ["all", "reversed", "one", "two"])
def test_mixed_batches_equal_the_restatement_file_by_file(emul, batch, S):
    """grey, 4:4:4, 4:2:2 and 4:2:0, every restart-interval case and the two saturating files in one batch: coefficients, entry states,
    block counts, per-file rounds and pixels are the single file's, and the batch takes the rounds of its slowest file"""
    names = BATCHES[batch]
    res, (rounds, chunks) = run_batch(emul, [CASES[n] for n in names], S)
    assert mismatches(res, names, S) == []
    assert chunks == 1 and rounds == max(DC.reference(n, S).rounds for n in names)


def test_the_case_list_holds_the_shapes_a_work_list_can_go_wrong_at():
    """A guard on the case list, not on the code (it holds without the feature): the batches of this file and of the GPU half lean on
    these shapes being there -- a file of fewer subsequences than a workgroup next to one that spans several, a file of one MCU, a last
    workgroup that is partial in every list"""
    sub = {n: DC.reference(n, 256).subsequences for n in CASES}
    assert sub[WIDE] > 512 and sub[WIDE] % 256 and 256 < sub[NOISE] < 512 and min(sub.values()) == 1
    assert DC.reference("size_8x8_444", 256).info.nmcu == 1
    assert any(DC.reference(n, 256).info.nblocks % 32 for n in CASES) and any(DC.reference(n, 256).info.nblocks > 256 for n in CASES)


def test_convergence_spread_leaves_the_early_files_exact(emul):
    """one file of hundreds of rounds beside files of two or three: the early ones rest from their first quiet round on, and their exit
    buffers, counts and parity are still theirs when the last pass runs hundreds of rounds later"""
    names = BATCHES["spread"]
    want = [DC.reference(n, 256).rounds for n in names]
    assert max(want) == DC.reference(NOISE, 256).rounds > 200 and sorted(want)[-3] <= 8
    assert any((w - max(want)) % 2 for w in want)  # (a parity that is not the batch's)
    res, (rounds, _) = run_batch(emul, [CASES[n] for n in names], 256)
    assert mismatches(res, names, 256) == [] and rounds == max(want)


def test_error_isolation(emul):
    """a damaged and an unsupported file in the middle of a good batch get their own status and position; the others are exact"""
    bad_parse, bad_pass = DC.corrupt_cases()["rst1_for_rst0"][0], DC.corrupt_cases()["one_block_too_few"][0]
    unsup = DC.unsupported_cases()["progressive"]
    good = ["size_17x17_420", WIDE, "dri1_444", "flat_gray_200", "midrow_420_r3"]
    files = [CASES[good[0]], CASES[good[1]], bad_pass, unsup, CASES[good[2]], bad_parse, CASES[good[3]], CASES[good[4]]]
    for S in (256, 1024):
        res, (rounds, chunks) = run_batch(emul, files, S)
        assert [r.status for r in res] == [0, 0, 3, 1, 0, 2, 0, 0]
        assert res[2].report[3] != 0xFFFFFFFF and res[3].error_pos > 0 and res[5].error_pos > 0
        assert mismatches([res[i] for i in (0, 1, 4, 6, 7)], good, S) == []
        assert rounds == max(DC.reference(n, S).rounds for n in good) and chunks == 1
    # every corrupt and unsupported case in the middle of a pair
    for name, data in {**{n: d for n, (d, _) in DC.corrupt_cases().items()}, **DC.unsupported_cases()}.items():
        res, _ = run_batch(emul, [CASES["dri1_444"], data, CASES["size_17x17_420"]], 256)
        assert res[1].status in (1, 2, 3), name
        assert mismatches([res[0], res[2]], ["dri1_444", "size_17x17_420"], 256) == [], name


def test_chunks_under_a_workspace_budget(emul):
    names = ["size_17x17_420", WIDE, "dri1_444", "flat_420", NOISE, "size_8x8_gray", "midrow_420_r3"]
    files = [CASES[n] for n in names]
    ws = [emul.jdecb_workspace(d, len(d), 256) for d in files]
    assert all(ws)
    def greedy(budget):
        """files in order while their sum stays within the budget; a file above it is a chunk of its own"""
        ends, total = [], 0
        for i, w in enumerate(ws):
            if total and total + w > budget:
                ends.append(i)
                total = 0
            total += w
        return ends + [len(ws)]

    budget = next(b for b in sorted({sum(ws[i:j]) for i in range(len(ws)) for j in range(i + 1, len(ws) + 1)}) if len(greedy(b)) == 3)
    ends = greedy(budget)
    assert len(ends) == 3 and max(ws) <= budget
    res, (rounds, chunks) = run_batch(emul, files, 256, budget)
    assert chunks == 3 and mismatches(res, names, 256) == []
    r = [DC.reference(n, 256).rounds for n in names]
    assert rounds == max(r[:ends[0]]) + max(r[ends[0]:ends[1]]) + max(r[ends[1]:])
    # a budget below every file: every file a chunk of its own
    res, (rounds, chunks) = run_batch(emul, files, 256, 1)
    assert chunks == len(names) and rounds == sum(r) and mismatches(res, names, 256) == []


# ---- the design broken on purpose ---------------------------------------------------------------------------------------------------
def _broken(tmp_path, how, batches):
    lib = _build(tmp_path / f"libbreak{how}.so", f"-DJDEC_BREAK={how}")
    out = {}
    for b in batches:
        names = BATCHES[b]
        res, _ = run_batch(lib, [CASES[n] for n in names], 256)
        out[b] = mismatches(res, names, 256)
        print(f"break {how}, batch {b}: {len(out[b])} of {len(names)} files differ")
    return out


@pytest.mark.parametrize("how", [1, 3])
def test_a_broken_design_fails_these_tests(tmp_path, how):
    """1: the round-(r - 1) flag slot reused for the skip decision (two slots, as in the single call): the file's first lane clears the
    slot the file's later workgroups read, so they rest while the first one runs; 3: the work lists off by one workgroup at every other
    file boundary.  Each must show in every batch above that has a file of several workgroups, or more than one file."""
    for b, bad in _broken(tmp_path, how, ("all", "two", "spread")).items():
        assert bad, (how, b)


def test_the_batchs_last_round_as_every_files_parity_changes_nothing(tmp_path):
    """2: the last pass reading every file's exit states by the parity of the BATCH's last round.  At a file's quiet round no entry state
    changed, so its two exit buffers agree in every state the last pass reads (they differ only in the last subsequence of a segment,
    whose exit nobody enters by), and a resting file's buffers stay as they are: the wrong parity reads the same states.  The per-file
    parity is kept because it is what the single call does and costs one word per file, not because a test can tell the difference --
    what protects a converged file is that it rests (break 1)."""
    assert _broken(tmp_path, 2, ("all", "spread")) == {"all": [], "spread": []}


# ---- sanitizers -----------------------------------------------------------------------------------------------------------------------
def test_standalone_sanitizer_run(tmp_path):
    """the host build as a program of its own under the address and undefined-behaviour sanitizers: the mixed batch with the corrupt and
    the unsupported files and every damaged scan of tests/jpgdmg_cases.py in it, forwards, reversed and cut into chunks; any report
    fails the run"""
    exe = tmp_path / "jpegdec_batch_san"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fno-fast-math", "-DJDEC_MAIN", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(HARNESS)], check=True,
                   capture_output=True, timeout=600)
    files = {}
    groups = (("ok", CASES), ("unsup", DC.unsupported_cases()), ("bad", {n: d for n, (d, _) in DC.corrupt_cases().items()}))
    names = [(g, n, d) for g, cases in groups for n, d in cases.items()]
    for k, (group, name, data) in enumerate(sorted(names, key=lambda t: zlib.crc32(t[1].encode()))):  # (a fixed order, the damaged ones among the good ones)
        p = tmp_path / f"{group}_{name}.jpg"
        p.write_bytes(data)
        files[str(p)] = group
    base = CASES["midrow_420_r3"]
    for n in list(range(0, 700, 37)) + list(range(700, len(base), 211)):
        p = tmp_path / f"cut_{n}.jpg"
        p.write_bytes(base[:n])
        files[str(p)] = "cut"
    # the damaged scans of tests/jpgdmg_cases.py, which do reach the entropy decoder: every file's status is the restatement's class
    for k, x in enumerate(M.sequential_cases()):
        p = tmp_path / f"dmg_{k}.jpg"
        p.write_bytes(x.data)
        files[str(p)] = M.verdict(x.name, 256, False).what
    r = subprocess.run([str(exe), *files], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = [l for l in r.stdout.strip().splitlines() if not l.startswith("batch ")]
    assert len(lines) == 2 * 3 * len(files)
    for line in lines:
        path, rc = line.split(" S=")[0], int(line.split("rc=")[1].split()[0])
        assert rc in {"ok": (0,), "unsup": (1,), "bad": (2, 3), "cut": (2, 3), "decoded": (0,), "unsupported": (1,), "parse": (2,),
                      "refused": (3,)}[files[path]], line
    chunks = [int(l.split("chunks=")[1]) for l in r.stdout.splitlines() if l.startswith("batch ")]
    assert chunks[0] == chunks[1] == 1 and chunks[2] > 3


# ---- the kernels' resources -----------------------------------------------------------------------------------------------------------
def test_batched_kernels_use_no_scratch_and_spill_nothing(tmp_path, product_lib):
    from test_resource_budget import kernel_metadata

    obj = ROOT / "vr180_convert_amd" / "csrc" / "kernels_jpegdec_batch.o"
    assert obj.exists(), "kernels_jpegdec_batch.o is built by __graft_entry__.build() / make"
    kernels = kernel_metadata(tmp_path, obj)
    assert len(kernels) == 8 and all("k_jdecb_" in k[".name"] for k in kernels)
    bad = [(k[".name"], k[".private_segment_fixed_size"], k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for k in kernels
           if k[".private_segment_fixed_size"] or k[".sgpr_spill_count"] or k[".vgpr_spill_count"]]
    assert not bad, bad
    assert all(k[".wavefront_size"] == 64 for k in kernels)


# ---- the library without a device -----------------------------------------------------------------------------------------------------
def test_batch_argument_checks_without_device(product_lib):
    lib = product_lib
    vp = C.c_void_p
    lib.v1c_jpeg_decode_batch.argtypes = [C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, C.c_uint32, C.c_uint64, vp, vp, vp]
    rounds = C.c_uint32(7)
    assert lib.v1c_jpeg_decode_batch(0, None, 0, None, None, None, None, None, 0, 0, None, None, C.byref(rounds)) == 0 and rounds.value == 0
    assert lib.v1c_jpeg_decode_batch(0, None, -1, None, None, None, None, None, 0, 0, None, None, None) == -1
    assert lib.v1c_jpeg_decode_batch(0, None, 1, None, None, None, None, None, 0, 0, None, None, None) == -1
    assert b"NULL" in lib.v1c_last_error()
    assert lib.v1c_jpeg_decode_batch(0, None, 1, None, None, None, None, None, 300, 0, None, None, None) == -1  # (NULL arrays first)
    one = (vp * 1)(None)
    assert lib.v1c_jpeg_decode_batch(0, None, 1, one, one, one, one, one, 300, 0, one, one, None) == -1 and b"subseq_bits" in lib.v1c_last_error()
    assert lib.v1c_jpeg_decode_batch(-1, None, 1, one, one, one, one, one, 0, 0, one, one, None) == -4
    assert lib.v1c_jpeg_decode_batch(64, None, 1, one, one, one, one, one, 0, 0, one, one, None) == -4
    # (device and stream capture are looked at before any file is: the per-file statuses are tested on the device)


# ---- Python plumbing, the native call stubbed -----------------------------------------------------------------------------------------
def _fake_single(J):
    def fake(path, **kw):
        name = Path(path).name
        if name == "p.jpg":
            raise NotImplementedError("progressive")
        if name == "bad.jpg":
            raise J.CorruptJPEG("damaged")
        if name == "gone.jpg":
            raise FileNotFoundError(name)
        if name == "bug.jpg":
            raise ValueError("an argument error")
        return "tensor of " + name

    return fake


def test_read_inputs_batch_hands_back_what_the_loop_does(monkeypatch, caplog):
    from vr180_convert_amd import jpeg_decode_device as J

    single = _fake_single(J)
    calls = []

    def many(paths, **kw):
        calls.append(([Path(p).name for p in paths], kw))
        out = []
        for p in paths:
            try:
                out.append(single(p))
            except Exception as e:  # noqa: BLE001
                out.append(e)
        return out

    monkeypatch.setattr(J, "imread_tensor", single)
    monkeypatch.setattr(J, "imread_tensors", many)
    arr = np.zeros((2, 2, 3), np.uint8)
    items = ["a.jpg", Path("p.jpg"), "bad.jpg", "gone.jpg", "x.png", arr]
    with caplog.at_level(logging.INFO, logger=J.LOG.name):
        want = J.read_inputs(items)
    loop = [(r.levelno, r.getMessage()) for r in caplog.records]
    caplog.clear()
    with caplog.at_level(logging.INFO, logger=J.LOG.name):
        got = J.read_inputs(items, batch=True)
    assert [(r.levelno, r.getMessage()) for r in caplog.records] == loop and len(loop) == 3
    assert got[:5] == want[:5] == ["tensor of a.jpg", Path("p.jpg"), "bad.jpg", "gone.jpg", "x.png"] and got[5] is arr
    assert calls == [(["a.jpg", "p.jpg", "bad.jpg", "gone.jpg"], {"device": None, "errors": "return"})]  # one call, eligible paths only
    with pytest.raises(ValueError, match="argument"):
        J.read_inputs(["a.jpg", "bug.jpg"], batch=True)
    calls.clear()
    assert J.read_inputs(["x.png", arr], batch=True)[1] is arr and calls == []


def test_errors_return_keeps_positions_and_errors_raise_raises_the_first(monkeypatch):
    """files the host parse refuses never reach the engine; the engine's per-file status lands in the file's own place"""
    import torch

    import vr180_convert_amd as V
    from vr180_convert_amd import _abi, _native, jpeg_decode_device as J

    assert V.decode_jpeg_tensors is J.decode_jpeg_tensors and V.imread_tensors is J.imread_tensors and V.last_batch_report is J.last_batch_report
    seen = {}

    real = _native.lib()

    class Lib:
        def __getattr__(self, name):
            return getattr(real, name)

        @staticmethod
        def v1c_jpeg_decode_batch(dev, stream, n, files, sizes, outs, pitches, cns, S, budget, status, reports, rounds):
            seen.update(n=n, sizes=list(sizes), pitches=list(pitches), S=S, budget=budget)
            for k in range(n):
                reports[k].segments, reports[k].subsequences, reports[k].rounds, reports[k].reserved = 1, 5 + k, 2 + k, k // 2
            status[1] = _abi.E_CORRUPT
            reports[1].error_pos = 77
            rounds._obj.value = 9
            return 0

    monkeypatch.setattr(J._native, "lib", lambda: Lib())
    monkeypatch.setattr(J, "_device", lambda device=None: torch.device("cpu"))
    monkeypatch.setattr(J, "_stream_ptr", lambda dev: None)
    good, grey = CASES["size_17x17_420"], CASES["size_8x8_gray"]
    items = [good, DC.unsupported_cases()["progressive"], grey, DC.corrupt_cases()["no_eoi"][0], good]
    single_before = J.last_decode_report()
    got = J.decode_jpeg_tensors(items, errors="return", subseq_bits=256, max_workspace_bytes=1 << 20)
    assert seen == dict(n=3, sizes=[len(good), len(grey), len(good)], pitches=[51, 24, 51], S=256, budget=1 << 20)
    assert tuple(got[0].shape) == (17, 17, 3) and tuple(got[4].shape) == (17, 17, 3)
    assert isinstance(got[1], NotImplementedError) and isinstance(got[3], J.CorruptJPEG)
    assert isinstance(got[2], J.CorruptJPEG) and "bit 77" in str(got[2])
    rep = J.last_batch_report()
    assert rep["batch_rounds"] == 9 and rep["chunks"] == 2
    assert rep["files"] == [dict(segments=1, subsequences=5, rounds=2, path="device"), None, None, None,
                            dict(segments=1, subsequences=7, rounds=4, path="device")]
    assert J.last_decode_report() == single_before
    with pytest.raises(NotImplementedError):
        J.decode_jpeg_tensors(items)
    with pytest.raises(J.CorruptJPEG, match="bit 77"):
        J.decode_jpeg_tensors([good, grey])
    assert J.decode_jpeg_tensors([]) == [] and J.last_batch_report() == dict(batch_rounds=0, chunks=0, files=[])
    with pytest.raises(ValueError):
        J.decode_jpeg_tensors([good], errors="ignore")
    with pytest.raises(ValueError):
        J.decode_jpeg_tensors([good], subseq_bits=100)


def test_device_decode_batch_reaches_read_inputs_with_batch(tmp_path, monkeypatch):
    import torch

    from vr180_convert_amd import _io, jpeg_decode_device, remapper

    calls = []

    def fake_read_inputs(items, **kw):
        calls.append(([Path(q).name for q in items], kw))
        return [torch.zeros((4, 8 if "sbs" in Path(q).name else 4, 3), dtype=torch.uint8) for q in items]

    monkeypatch.setattr(jpeg_decode_device, "read_inputs", fake_read_inputs)
    monkeypatch.setattr(_io, "imread_many", lambda paths: list(paths))
    monkeypatch.setattr(_io, "imwrite", lambda p, a: True)
    monkeypatch.setattr(_io, "imwrite_many", lambda ps, ims: None)
    monkeypatch.setattr(remapper, "_to_device", lambda im, dev: im)
    monkeypatch.setattr(remapper, "_device", lambda device=None: torch.device("cpu"))
    monkeypatch.setattr(remapper, "_radius_for_pair", lambda *a: 1.0)
    seen = []
    monkeypatch.setattr(remapper, "apply_lr_tensors", lambda t, l, r, **k: seen.append((tuple(l.shape), tuple(r.shape))) or
                        torch.zeros((4, 8, 3), dtype=torch.uint8))

    def lr(left, right, **kw):
        calls.clear(), seen.clear()
        remapper.apply_lr(None, left_path=tmp_path / left, right_path=tmp_path / right, out_path=tmp_path / "o.png", size_output=(4, 4), **kw)
        return list(calls)

    assert lr("l.jpg", "r.jpg", device_decode="batch") == [(["l.jpg", "r.jpg"], {"device": None, "batch": True})]  # L and R: one batch
    assert lr("l.jpg", "r.jpg", device_decode=True) == [(["l.jpg", "r.jpg"], {"device": None})]
    assert lr("sbs.jpg", "sbs.jpg", device_decode="batch") == [(["sbs.jpg"], {"device": None, "batch": True})]   # decoded once
    assert seen == [((4, 4, 3), (4, 4, 3))]
    with pytest.raises(ValueError, match="batch"):
        lr("l.jpg", "r.jpg", device_decode="all")

    monkeypatch.setattr(remapper, "get_radius_smart", lambda r, ims: 1.0)
    monkeypatch.setattr(remapper, "remap_tensors", lambda *a, **k: None)
    monkeypatch.setattr(remapper.torch, "empty", lambda shape, dtype=None, device=None: torch.zeros(shape, dtype=torch.uint8))
    monkeypatch.setattr(remapper._hostpipe, "enabled", lambda *a: False)
    calls.clear()
    remapper.apply(None, in_paths=[tmp_path / "a.jpg", tmp_path / "b.jpg", tmp_path / "c.jpg"], size_output=(4, 4), device_decode="batch")
    assert calls == [(["a.jpg", "b.jpg", "c.jpg"], {"device": None, "batch": True})]


def test_cli_batch_flag_reaches_apply_and_apply_lr(tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from vr180_convert_amd import _io, cli, remapper, synth

    seen = []
    monkeypatch.setattr(remapper, "apply_lr", lambda *a, **k: seen.append(("lr", k.get("device_decode"))))
    monkeypatch.setattr(remapper, "apply", lambda *a, **k: seen.append(("s", k.get("device_decode"))))
    img = tmp_path / "a.png"
    _io.imwrite(img, synth.pattern(64, 64))
    run = CliRunner().invoke
    base = ["--radius", "max", "--size", "32x32", "--out-path", str(tmp_path / "o.jpg")]
    assert run(cli.app, ["lr", str(img), str(img), *base, "--device-decode-batch"]).exit_code == 0
    assert run(cli.app, ["s", str(img), *base, "--device-decode-batch"]).exit_code == 0
    assert run(cli.app, ["s", str(img), *base, "--device-decode"]).exit_code == 0
    assert seen == [("lr", "batch"), ("s", "batch"), ("s", True)]
