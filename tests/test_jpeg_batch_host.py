"""The batched device JPEG encoder without a GPU: a sequential host copy of its decomposition (tests/host_jpeg_batch/, built from the
product's headers, jpeg_batch.hpp included) against the restatement file by file, byte for byte; the cut into chunks; the work lists;
the copy broken on purpose; the stand-alone sanitizer run; the resource budget of kernels_jpeg_batch.o; the C ABI's argument checks;
the Python plumbing with the native call stubbed."""
import ctypes as C
import functools
import re
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

import jpg_cases as PC
import jpg_ref as R

ROOT = Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "host_jpeg_batch" / "jpeg_batch_emul.hip"
CASES = PC.shared_cases()
NAMES = list(CASES)
TRIPLE = "noise_gray_q100_r1"  # 64 one-block intervals, pads on byte boundaries, a padded last byte of 0xFF
TILE, BLOCK, PIECE = 0, 1, 2   # the work lists of jpeg_batch.hpp
PER_GROUP = {TILE: 32, BLOCK: 256, PIECE: 256}


class EmulImage(C.Structure):
    _fields_ = [("img", C.c_void_p), ("h", C.c_int32), ("w", C.c_int32), ("pitch", C.c_int64), ("cn", C.c_int32), ("quality", C.c_int32),
                ("subsampling", C.c_int32), ("restart_mcus", C.c_int32), ("coef", C.c_void_p), ("bits", C.c_void_p), ("file", C.c_void_p),
                ("capacity", C.c_uint64), ("size", C.c_uint64)]


def _build(out, *flags):
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-fno-fast-math", *flags, "-o", str(out),
                    str(HARNESS)], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(out))
    lib.jpegb_emul_workspace.argtypes = [C.c_int] * 5
    lib.jpegb_emul_workspace.restype = C.c_uint64
    lib.jpegb_emul_default_budget.restype = C.c_uint64
    lib.jpegb_emul_file_of.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.jpegb_emul_file_of.restype = C.c_uint32
    lib.jpegb_emul_tables.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.jpegb_emul_encode.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("host_jpeg_batch") / "libjpeg_batch_emul.so")


# beyond the shared cases (none of which has more than 252 blocks): images of several workgroups in the 256-block list too, with partial
# last ones in every list -- 969 and 342 blocks
LARGER = {"larger_444_r5": lambda: PC.dense(PC.noise(136, 152, 3, 7) // 2 + PC.smooth(136, 152, 3, 8) // 2, 90, "444", 5),
          "larger_gray": lambda: PC.dense(PC.smooth(150, 141, 1, 9), 95)}


@functools.lru_cache(maxsize=None)
def _case(name):
    return CASES[name] if name in CASES else LARGER[name]()


@functools.lru_cache(maxsize=None)
def _reference(name):
    if name in CASES:
        return PC.reference(name)
    c = _case(name)
    img = np.ascontiguousarray(c.image())
    zz = R.coefficients(img, c.quality, c.subsampling)
    return zz, R.block_bits(zz, R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart)), R.encode(img, c.quality, c.subsampling, c.restart)


def _images(names):
    images = (EmulImage * len(names))()
    keep = []
    for k, name in enumerate(names):
        c = _case(name)
        g = R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart)
        coef, bits = np.zeros((g.nblocks, 64), np.int16), np.zeros(g.nblocks, np.uint32)
        out = np.zeros(R.bound(c.h, c.w, c.cn, c.subsampling, c.restart) + 1024 + 2, np.uint8)
        images[k] = EmulImage(c.base.ctypes.data + c.offset, c.h, c.w, c.pitch, c.cn, c.quality, R.SUBSAMPLINGS[c.subsampling], c.restart,
                              coef.ctypes.data, bits.ctypes.data, out.ctypes.data, out.size, 0)
        keep.append((coef, bits, out))
    return images, keep


def _run(lib, names, budget=0):
    """the batch through the harness: (names whose coefficients, block bits or file differ from the restatement, chunks)"""
    images, keep = _images(names)
    chunks = C.c_uint32(0)
    rc = lib.jpegb_emul_encode(len(names), images, budget, C.byref(chunks))
    assert rc == 0, rc
    wrong = []
    for k, name in enumerate(names):
        zz, wbits, wdata = _reference(name)
        coef, bits, out = keep[k]
        data = out[:images[k].size].tobytes()
        if not (np.array_equal(coef, zz) and np.array_equal(bits, wbits) and data == wdata):
            wrong.append((k, name))
    return wrong, chunks.value


def _workspace(lib, name):
    c = _case(name)
    return lib.jpegb_emul_workspace(c.h, c.w, c.cn, R.SUBSAMPLINGS[c.subsampling], c.restart)


def _chunk_ends(bytes_, budget):
    """chunk_ends of jpegdec_batch.hpp, restated: files in order while their sum stays within the budget; a larger one by itself (the
    workgroup limit of 2^31 - 1 is far from these sizes)"""
    ends, total, start = [], 0, 0
    for f, b in enumerate(bytes_):
        if f > start and total + b > budget:
            ends.append(f)
            start, total = f, 0
        total += b
    return ends + [len(bytes_)] if bytes_ else ends


# ---- byte equality ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["in_order", "reversed", "triple"])
def test_every_file_of_a_batch_is_the_restatements(emul, variant):
    names = {"in_order": NAMES, "reversed": NAMES[::-1], "triple": [TRIPLE] * 3}[variant]
    assert len(NAMES) == 48
    wrong, chunks = _run(emul, names)
    assert wrong == [] and chunks == 1


def test_every_case_as_a_batch_of_one(emul):
    for name in NAMES:
        assert _run(emul, [name]) == ([], 1), name


def test_images_of_several_workgroups_in_every_list(emul):
    names = ["size_7x9_gray", "larger_444_r5", "flat", "larger_gray", "larger_444_r5", "size_1x1_420"]
    for n, blocks in (("larger_444_r5", 969), ("larger_gray", 342)):
        c = _case(n)
        assert R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart).nblocks == blocks
    assert _run(emul, names) == ([], 1)
    budget = _workspace(emul, "larger_444_r5") + _workspace(emul, "flat")
    assert _chunk_ends([_workspace(emul, n) for n in names], budget) == [2, 4, 6]
    assert _run(emul, names, budget) == ([], 3)


def test_the_triple_puts_an_image_end_in_front_of_an_image_start_at_every_kind_of_pad():
    """a guard on the case the triple leans on, not on the code: intervals that end on a byte (no pad), that are padded, and whose padded
    last byte is 0xFF -- the last interval of the image, which the next image follows, is one of the 64"""
    iv = PC.intervals(TRIPLE)
    assert len(iv) == 64 and any(n % 8 == 0 for n, _ in iv) and any(n % 8 and b[-1] == 0xFF for n, b in iv) and any(n % 8 and b[-1] != 0xFF for n, b in iv)


# ---- the workspace budget -----------------------------------------------------------------------------------------------------------
def test_chunks_under_a_workspace_budget(emul):
    ws = [_workspace(emul, n) for n in NAMES]
    assert min(ws) > 0 and emul.jpegb_emul_default_budget() == 1 << 30
    # the worst-case regions of the single call -- coef 128, raw 208 and out 416 bytes per block, 752 together -- with the block and
    # piece counters and their scans (12 bytes per block, 12 per 16-byte piece of raw: 168), and a fixed share of the chunk's head
    for n, b in zip(NAMES, ws):
        c = CASES[n]
        g = R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart)
        assert 920 * g.nblocks <= b <= 920 * g.nblocks + 20 * g.nint + 8192, (n, b, g.nblocks)
    several = sum(ws) // 5
    assert several > max(ws)
    wrong, chunks = _run(emul, NAMES, several)
    assert wrong == [] and chunks == len(_chunk_ends(ws, several)) and 5 <= chunks <= 10
    tiny = max(ws) - 1  # smaller than the largest case: that one is a chunk of its own
    wrong, chunks = _run(emul, NAMES, tiny)
    ends = _chunk_ends(ws, tiny)
    big = ws.index(max(ws))
    assert wrong == [] and chunks == len(ends) and big + 1 in ends and (big == 0 or big in ends)
    wrong, chunks = _run(emul, NAMES, 1)  # every image by itself
    assert wrong == [] and chunks == len(NAMES)


# ---- the work lists -----------------------------------------------------------------------------------------------------------------
def test_work_lists_tile_every_list_and_no_workgroup_crosses_an_image(emul):
    n = len(NAMES)
    images, _keep = _images(NAMES)
    first = np.zeros((3, n + 1), np.uint32)
    regions = np.zeros((n, 8), np.uint64)
    assert emul.jpegb_emul_tables(n, images, first.ctypes.data, regions.ctypes.data) == 3
    blk0, int0, piece0, out0, nblocks, nint, pieces, bound = (regions[:, k].astype(np.int64) for k in range(8))
    for k, name in enumerate(NAMES):
        c = CASES[name]
        g = R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart)
        assert (nblocks[k], nint[k], bound[k]) == (g.nblocks, g.nint, R.bound(c.h, c.w, c.cn, c.subsampling, c.restart))
        assert pieces[k] * 16 >= g.nblocks * 208 + g.nint > (pieces[k] - 1) * 16
    # the regions lie back to back, in order, and a raw region starts on a piece (piece0 counts pieces)
    for start, size in ((blk0, nblocks), (int0, nint), (piece0, pieces), (out0, bound)):
        assert start[0] == 0 and np.array_equal(start[1:], np.cumsum(size)[:-1])
    counts = {TILE: nblocks, BLOCK: nblocks, PIECE: pieces}
    for lst in (TILE, BLOCK, PIECE):
        f1 = first[lst].astype(np.int64)
        per = PER_GROUP[lst]
        groups = -(-counts[lst] // per)
        assert f1[0] == 0 and np.array_equal(np.diff(f1), groups) and groups.min() >= 1       # the ranges tile the list
        ptr = first[lst].ctypes.data
        for k in range(n):
            for wg in {int(f1[k]), int(f1[k + 1]) - 1}:                                          # every image's first and last workgroup
                assert emul.jpegb_emul_file_of(ptr, n, wg) == k, (lst, k, wg)
            # the last workgroup's range ends inside the image's own entries: it is partial or exact, never beyond
            last = int(f1[k + 1] - 1 - f1[k])
            assert last * per < counts[lst][k] <= (last + 1) * per
        for wg in range(int(f1[n])):                                                             # every workgroup has one image
            k = emul.jpegb_emul_file_of(ptr, n, wg)
            assert f1[k] <= wg < f1[k + 1]
    assert any(nblocks[k] % 32 and nblocks[k] > 32 for k in range(n)) and any(pieces[k] % 256 and pieces[k] > 256 for k in range(n))
    assert (nint <= nblocks).all()                                                               # the interval kernel rides the block list


# ---- the harness broken on purpose --------------------------------------------------------------------------------------------------
# cases of the 48-case batch (in order) that fail, measured on the host build
BREAKS = {1: "the DC predecessor carried over an image boundary", 2: "RSTm numbered over the batch",
          3: "the image's base not subtracted from ffoff in the placement"}


@pytest.mark.parametrize("how", sorted(BREAKS))
def test_a_broken_decomposition_fails_byte_equality(tmp_path, how):
    """1 fails every image but the first whose first DC differs from the coefficient in front of it; 2 every image of more than one
    interval whose first interval is not a multiple of eight intervals into the batch; 3 every image behind the first 0xFF byte of the
    batch.  Measured (of 48, in order / reversed): 1: 46 / 46, 2: 31 / 30, 3: 44 / 47."""
    lib = _build(tmp_path / f"libbreak{how}.so", f"-DJPEGB_BREAK={how}")
    counts = []
    for names in (NAMES, NAMES[::-1]):
        wrong, _ = _run(lib, names)
        counts.append(len(wrong))
        assert wrong and wrong[0][0] > 0  # (the first image has nothing in front of it)
    print(f"break {how} ({BREAKS[how]}): {counts[0]} of 48 in order, {counts[1]} reversed")
    wrong, _ = _run(lib, [TRIPLE] * 3)
    assert [k for k, _ in wrong] == ([1, 2] if how != 2 else [])  # (64 intervals: a multiple of eight, RSTm stays in step)


# ---- sanitizers ---------------------------------------------------------------------------------------------------------------------
def test_standalone_sanitizer_run(tmp_path, emul):
    """the harness as a program of its own under the address and undefined-behaviour sanitizers: the 48-case batch in one chunk and
    under a budget that makes every image a chunk; any report fails the run, and the files are the restatement's"""
    exe = tmp_path / "jpeg_batch_san"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fno-fast-math", "-DJPEGB_MAIN", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(HARNESS)], check=True,
                   capture_output=True, timeout=600)
    lines = []
    for name in NAMES:
        c = CASES[name]
        p = tmp_path / f"{name}.raw"
        p.write_bytes(c.base.tobytes())
        lines.append(f"{c.h} {c.w} {c.cn} {c.pitch} {c.quality} {R.SUBSAMPLINGS[c.subsampling]} {c.restart} {c.offset} {p}")
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    several = sum(_workspace(emul, n) for n in NAMES) // 5
    r = subprocess.run([str(exe), str(tmp_path / "list.txt"), "0", "1", str(several)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out = r.stdout.strip().splitlines()
    batches = [l for l in out if l.startswith("batch ")]
    assert [int(l.split("chunks=")[1]) for l in batches] == [1, 48, len(_chunk_ends([_workspace(emul, n) for n in NAMES], several))]
    files = [l for l in out if l.startswith("image ")]
    assert len(files) == 3 * 48
    for l in files:
        k = int(l.split()[1])
        data = PC.reference(NAMES[k])[2]
        assert l.split()[2:] == [f"size={len(data)}", f"crc={zlib.crc32(data):08x}"], l


# ---- the kernels' resources ---------------------------------------------------------------------------------------------------------
def _short(kernel):
    return re.search(r"k_jpegb?_([a-z_]+)E", kernel[".name"]).group(1)


def test_batched_kernels_use_no_scratch_and_spill_nothing(tmp_path, product_lib):
    from test_resource_budget import kernel_metadata

    csrc = ROOT / "vr180_convert_amd" / "csrc"
    assert (csrc / "kernels_jpeg_batch.o").exists(), "kernels_jpeg_batch.o is built by __graft_entry__.build() / make"
    (tmp_path / "batch").mkdir(), (tmp_path / "single").mkdir()
    kernels = kernel_metadata(tmp_path / "batch", csrc / "kernels_jpeg_batch.o")
    assert all("k_jpegb_" in k[".name"] for k in kernels)
    assert sorted(_short(k) for k in kernels) == ["count", "interval_bytes", "pack", "place", "size", "transform"]
    bad = [(k[".name"], k[".private_segment_fixed_size"], k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for k in kernels
           if k[".private_segment_fixed_size"] or k[".sgpr_spill_count"] or k[".vgpr_spill_count"]]
    assert not bad, bad
    assert all(k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 256 for k in kernels)
    # LDS: what the single kernels use (a workgroup's descriptor lives in scalar registers)
    single = {_short(k): k[".group_segment_fixed_size"] for k in kernel_metadata(tmp_path / "single", csrc / "kernels_jpeg.o")}
    for k in kernels:
        print(_short(k), "VGPRs", k[".vgpr_count"], "SGPRs", k[".sgpr_count"], "LDS", k[".group_segment_fixed_size"], "single LDS", single[_short(k)])
        assert k[".group_segment_fixed_size"] <= single[_short(k)], (_short(k), k[".group_segment_fixed_size"], single[_short(k)])


# ---- the library without a device ---------------------------------------------------------------------------------------------------
def test_batch_argument_checks_without_device(product_lib):
    from vr180_convert_amd.jpeg_device import JpegImage

    lib = product_lib
    assert lib.v1c_abi_version() == 1
    lib.v1c_jpeg_bound.restype = C.c_uint64
    chunks = C.c_uint32(7)
    assert lib.v1c_jpeg_encode_batch(0, None, 0, None, 0, C.byref(chunks)) == 0 and chunks.value == 0
    assert lib.v1c_jpeg_encode_batch(0, None, -1, None, 0, None) == -1 and b"negative" in lib.v1c_last_error()
    assert lib.v1c_jpeg_encode_batch(0, None, 2, None, 0, None) == -1 and b"NULL" in lib.v1c_last_error()
    buf = np.zeros(1 << 16, np.uint8)  # stands in for the device pointer: validation fails before any device call
    out = np.zeros(1 << 20, np.uint8)
    assert lib.v1c_jpeg_bound(64, 64, 3, 2, 4) <= 1 << 20

    def call(k=2, **bad):
        images = (JpegImage * 4)()
        for i in range(4):
            images[i] = JpegImage(buf.ctypes.data, 64, 64, 192, 3, 95, 2, 4, out.ctypes.data, 1 << 20, 99)
        for name, v in bad.items():
            setattr(images[k], name, v)
        rc = lib.v1c_jpeg_encode_batch(0, None, 4, images, 0, None)
        assert [im.size for im in images] == [99] * 4  # nothing was touched
        return rc, lib.v1c_last_error().decode()

    for k, bad, word in [(2, {"cn": 2}, "cn"), (0, {"quality": 0}, "quality"), (3, {"quality": 101}, "quality"), (1, {"subsampling": 1}, "subsampling"),
                         (2, {"restart_mcus": 0}, "restart"), (2, {"restart_mcus": 65536}, "restart"), (3, {"h": 0}, "65535"),
                         (1, {"w": 65536, "pitch": 1 << 20}, "65535"), (2, {"img": None}, "NULL"), (0, {"out_host": None}, "NULL"),
                         (3, {"capacity": lib.v1c_jpeg_bound(64, 64, 3, 2, 4) - 1}, "capacity"), (1, {"pitch": 191}, "pitch")]:
        rc, msg = call(k, **bad)
        assert rc == -1 and f"image {k}:" in msg and word in msg, (bad, msg)


# ---- the Python plumbing, the native call stubbed -----------------------------------------------------------------------------------
class _FakeImage:
    """stands in for a CUDA uint8 tensor behind ``_image``"""

    def __init__(self, h, w, cn, device="cuda:0", ptr=0x1000):
        import torch

        self.shape, self.device, self.ptr = (h, w, cn), torch.device(device), ptr

    def stride(self, k):
        return (self.shape[1] * self.shape[2] + 5, self.shape[2], 1)[k]

    def data_ptr(self):
        return self.ptr


class _FakeLib:
    """the real library's host-only calls, and a recording stand-in for v1c_jpeg_encode_batch that writes image k's index as its scan"""

    def __init__(self, real):
        self.real, self.calls = real, []
        self.v1c_jpeg_bound, self.v1c_jpeg_header, self.v1c_last_error = real.v1c_jpeg_bound, real.v1c_jpeg_header, real.v1c_last_error

    def v1c_jpeg_encode_batch(self, dev, stream, n, images, budget, chunks):
        seen = []
        for k in range(n):
            im = images[k]
            assert im.capacity == self.real.v1c_jpeg_bound(im.h, im.w, im.cn, im.subsampling, im.restart_mcus)
            tag = len(self.calls) * 16 + k
            C.memmove(im.out_host, bytes([tag]) * (k + 3), k + 3)
            im.size = k + 3
            seen.append((im.img, im.h, im.w, im.pitch, im.cn, im.quality, im.subsampling, im.restart_mcus, im.out_host))
        self.calls.append((dev, n, budget, seen))
        chunks._obj.value = 2
        return 0


@pytest.fixture
def stubbed(monkeypatch, product_lib):
    import torch

    from vr180_convert_amd import _native
    from vr180_convert_amd import jpeg_device as J

    fake = _FakeLib(product_lib)
    monkeypatch.setattr(_native, "lib", lambda: fake)
    monkeypatch.setattr(J, "_image", lambda t: t if isinstance(t, _FakeImage) else (_ for _ in ()).throw(TypeError("the device JPEG encoder takes CUDA tensors")))
    monkeypatch.setattr(J, "_stream_ptr", lambda dev: 0)
    bufs = {}
    monkeypatch.setattr(J, "_host_buffer", lambda dev, n: bufs.setdefault(n, torch.zeros(max(n, 1), dtype=torch.uint8)))
    return J, fake


def test_scalar_and_sequence_parameters_reach_the_engine_per_image(stubbed):
    J, fake = stubbed
    ts = [_FakeImage(16, 24, 3, ptr=0x1000), _FakeImage(9, 9, 1, ptr=0x2000), _FakeImage(1, 40, 4, ptr=0x3000)]
    files = J.encode_jpeg_tensors(ts, quality=[95, 50, 1], subsampling=("420", "444", "420"), restart_mcus=[None, 3, None], workspace_budget=12345)
    (dev, n, budget, seen), = fake.calls
    assert (dev, n, budget) == (0, 3, 12345)
    assert [s[:8] for s in seen] == [(0x1000, 16, 24, 24 * 3 + 5, 3, 95, 2, 2), (0x2000, 9, 9, 14, 1, 50, 0, 3), (0x3000, 1, 40, 160, 4, 1, 2, 3)]
    assert seen[1][8] - seen[0][8] == fake.real.v1c_jpeg_bound(16, 24, 3, 2, 2)  # the landing regions lie back to back
    for k, (f, q, sub, r) in enumerate(zip(files, (95, 50, 1), ("420", "444", "420"), (2, 3, 3))):
        h, w, cn = ts[k].shape
        assert f == R.headers(R.Geom(h, w, cn, sub, r), q) + bytes([k]) * (k + 3) + b"\xff\xd9"
    assert J.last_encode_batch_report() == {"chunks": 2, "sizes": [3, 4, 5]}
    # scalars serve every image; the defaults are the single call's
    fake.calls.clear()
    J.encode_jpeg_tensors(ts[:2])
    assert [s[5:8] for s in fake.calls[0][3]] == [(95, 2, 2), (95, 2, 2)] and fake.calls[0][2] == 0
    J.encode_jpeg_tensors(ts[:2], quality=7, subsampling="444", restart_mcus=9)
    assert [s[5:8] for s in fake.calls[1][3]] == [(7, 0, 9), (7, 0, 9)]


def test_argument_errors_are_the_single_calls_and_come_before_the_native_call(stubbed):
    import torch

    J, fake = stubbed
    ts = [_FakeImage(16, 24, 3), _FakeImage(9, 9, 1)]
    assert J.encode_jpeg_tensors([]) == [] and J.last_encode_batch_report() == {"chunks": 0, "sizes": []}
    J.imwrite_jpeg_tensors([], [])
    for kw in ({"quality": [95]}, {"subsampling": ["420", "420", "420"]}, {"restart_mcus": [1, 2, 3]}, {"quality": [95, 0]}, {"quality": 101},
               {"subsampling": "422"}, {"subsampling": ["420", "411"]}, {"restart_mcus": [1, 65536]}, {"restart_mcus": 0}, {"workspace_budget": -1}):
        with pytest.raises(ValueError):
            J.encode_jpeg_tensors(ts, **kw)
    with pytest.raises(ValueError, match="one device"):
        J.encode_jpeg_tensors([_FakeImage(8, 8, 3, "cuda:0"), _FakeImage(8, 8, 3, "cuda:1")])
    with pytest.raises(ValueError, match="65535"):
        J.encode_jpeg_tensors([_FakeImage(8, 65536, 1)])
    with pytest.raises(TypeError):
        J.encode_jpeg_tensors([ts[0], torch.zeros((4, 4, 3), dtype=torch.uint8)])
    with pytest.raises(ValueError, match="paths"):
        J.imwrite_jpeg_tensors(["a.jpg"], ts)
    assert fake.calls == []


def test_a_list_beyond_the_pinned_budget_goes_in_sub_lists(stubbed, monkeypatch, tmp_path):
    J, fake = stubbed
    ts = [_FakeImage(16, 16, 3), _FakeImage(8, 8, 1), _FakeImage(8, 8, 1), _FakeImage(16, 16, 3), _FakeImage(8, 8, 1)]
    b = [fake.real.v1c_jpeg_bound(h, w, cn, 2, 1) for h, w, cn in (t.shape for t in ts)]
    assert b[0] > 2 * b[1]
    assert J.PINNED_BUDGET == 1 << 30 and J.sub_lists(b) == [(0, 5)] and J.sub_lists([]) == []
    assert J.sub_lists(b, b[0] + b[1]) == [(0, 2), (2, 4), (4, 5)]
    assert J.sub_lists(b, 1) == [(0, 1), (1, 3), (3, 4), (4, 5)]      # the budget is never below the largest single bound
    assert J.sub_lists([3 << 30, 5, 5], None) == [(0, 1), (1, 3)]
    monkeypatch.setattr(J, "PINNED_BUDGET", b[0] + b[1])
    paths = [tmp_path / f"{k}.jpg" for k in range(5)]
    J.imwrite_jpeg_tensors(paths, ts, restart_mcus=1)
    assert [(n, [s[1] for s in seen]) for _, n, _, seen in fake.calls] == [(2, [16, 8]), (2, [8, 16]), (1, [8])]
    assert J.last_encode_batch_report() == {"chunks": 6, "sizes": [3, 4, 3, 4, 3]}
    for k, (call, i) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)]):   # every file holds its own sub-list's scan
        h, w, cn = ts[k].shape
        assert paths[k].read_bytes() == R.headers(R.Geom(h, w, cn, "420", 1), 95) + bytes([call * 16 + i]) * (i + 3) + b"\xff\xd9"


class _FakeCuda:
    """stands in for a CUDA tensor where only the routing is under test"""

    def __init__(self, a):
        import torch

        self.a, self.dtype, self.is_cuda = a, {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16}[a.dtype], True

    def cpu(self):
        import torch

        return torch.from_numpy(self.a)

    def __getitem__(self, key):
        return self


def test_device_jpeg_batch_sends_the_eligible_results_in_one_call_in_order(tmp_path, monkeypatch):
    import torch

    from vr180_convert_amd import _io, jpeg_device, png_device, remapper

    batches, singles, png_writes, host_writes = [], [], [], []
    monkeypatch.setattr(jpeg_device, "eligible", lambda p, r: str(p).lower().endswith((".jpg", ".jpeg")) and getattr(r, "is_cuda", False)
                        and r.dtype == torch.uint8)
    monkeypatch.setattr(png_device, "eligible", lambda p, r: str(p).lower().endswith(".png") and getattr(r, "is_cuda", False))
    monkeypatch.setattr(jpeg_device, "imwrite_jpeg_tensors", lambda ps, ts, **k: batches.append(([Path(p).name for p in ps], list(ts))))
    monkeypatch.setattr(jpeg_device, "imwrite_jpeg_tensor", lambda p, t, **k: singles.append(Path(p).name))
    monkeypatch.setattr(png_device, "imwrite_tensor", lambda p, t, **k: png_writes.append(Path(p).name))
    monkeypatch.setattr(_io, "imwrite", lambda p, a: host_writes.append(Path(p).name) or True)
    monkeypatch.setattr(_io, "imwrite_many", lambda ps, ims: host_writes.extend(Path(p).name for p in ps))
    monkeypatch.setattr(_io, "imread_many", lambda paths: list(paths))
    monkeypatch.setattr(remapper, "_to_device", lambda im, dev: im)
    monkeypatch.setattr(remapper, "_device", lambda device=None: torch.device("cpu"))
    monkeypatch.setattr(remapper, "_radius_for_pair", lambda *a: 1.0)
    monkeypatch.setattr(remapper, "get_radius_smart", lambda r, ims: 1.0)
    monkeypatch.setattr(remapper, "remap_tensors", lambda *a, **k: None)
    made = []
    monkeypatch.setattr(remapper.torch, "empty", lambda shape, dtype=None, device=None: made.append(_FakeCuda(np.zeros(shape, np.uint8))) or made[-1])
    srcs = [_FakeCuda(np.zeros((4, 4, 3), np.uint8)) for _ in range(4)]
    for s_ in srcs:
        s_.shape, s_.device = (4, 4, 3), torch.device("cpu")

    def s(names, **kw):
        for log in (batches, singles, png_writes, host_writes, made):
            log.clear()
        remapper.apply(None, in_paths=srcs[:len(names)], out_paths=[tmp_path / n for n in names], size_output=(4, 4), **kw)
        return list(batches), list(singles), list(png_writes), list(host_writes)

    b, one, png, host = s(["a.jpg", "b.png", "c.JPEG", "d.npy"], device_jpeg="batch")
    assert [names for names, _ in b] == [["a.jpg", "c.JPEG"]] and b[0][1] == [made[0], made[2]]
    assert (one, png, host) == ([], [], ["b.png", "d.npy"])
    b, one, png, host = s(["a.jpg", "b.png", "c.JPEG", "d.npy"], device_jpeg="batch", device_png=True)
    assert [names for names, _ in b] == [["a.jpg", "c.JPEG"]] and (one, png, host) == ([], ["b.png"], ["d.npy"])
    assert s(["b.png", "d.npy"], device_jpeg="batch") == ([], [], [], ["b.png", "d.npy"])          # nothing eligible: no call
    assert s(["a.jpg", "b.png", "c.JPEG"], device_jpeg=True) == ([], ["a.jpg", "c.JPEG"], [], ["b.png"])  # the loop, as before
    for bad in ("maybe", "Batch", ""):
        if bad:
            with pytest.raises(ValueError, match="device_jpeg"):
                remapper.apply(None, in_paths=srcs[:1], out_paths=[tmp_path / "a.jpg"], size_output=(4, 4), device_jpeg=bad)
            with pytest.raises(ValueError, match="device_jpeg"):
                remapper.apply_lr(None, left_path=srcs[0], right_path=srcs[0], out_path=tmp_path / "a.jpg", size_output=(4, 4), device_jpeg=bad)

    # apply_lr: the side-by-side frame is a batch of one
    sbs = _FakeCuda(np.zeros((4, 8, 3), np.uint8))
    monkeypatch.setattr(remapper, "apply_lr_tensors", lambda *a, **k: sbs)
    img = np.zeros((4, 4, 3), np.uint8)

    def lr(name, **kw):
        for log in (batches, singles, png_writes, host_writes):
            log.clear()
        remapper.apply_lr(None, left_path=img, right_path=img, out_path=tmp_path / name, size_output=(4, 4), **kw)
        return list(batches), list(singles), list(png_writes), list(host_writes)

    assert lr("a.jpg", device_jpeg="batch") == ([(["a.jpg"], [sbs])], [], [], [])
    assert lr("a.jpg", device_jpeg=True) == ([], ["a.jpg"], [], [])
    assert lr("a.png", device_jpeg="batch") == ([], [], [], ["a.png"])
    assert lr("a.png", device_jpeg="batch", device_png=True) == ([], [], ["a.png"], [])


def test_cli_batch_flag_reaches_apply_and_apply_lr(tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from vr180_convert_amd import _io, cli, remapper, synth

    seen = []
    monkeypatch.setattr(remapper, "apply_lr", lambda *a, **k: seen.append(("lr", k.get("device_jpeg"))))
    monkeypatch.setattr(remapper, "apply", lambda *a, **k: seen.append(("s", k.get("device_jpeg"))))
    img = tmp_path / "a.png"
    _io.imwrite(img, synth.pattern(64, 64))
    run = CliRunner().invoke
    base = ["--radius", "max", "--size", "32x32", "--out-path", str(tmp_path / "o.jpg")]
    assert run(cli.app, ["lr", str(img), str(img), *base, "--device-jpeg-batch"]).exit_code == 0
    assert run(cli.app, ["lr", str(img), str(img), *base, "--device-jpeg-batch", "--device-jpeg"]).exit_code == 0   # the batch wins
    assert run(cli.app, ["lr", str(img), str(img), *base, "--device-jpeg"]).exit_code == 0
    assert run(cli.app, ["s", str(img), *base, "--device-jpeg-batch"]).exit_code == 0
    assert run(cli.app, ["s", str(img), *base, "--device-jpeg", "--device-jpeg-batch"]).exit_code == 0
    assert run(cli.app, ["s", str(img), *base]).exit_code == 0
    assert seen == [("lr", "batch"), ("lr", "batch"), ("lr", True), ("s", "batch"), ("s", "batch"), ("s", None)]


def test_exports():
    import vr180_convert_amd as V
    from vr180_convert_amd import jpeg_device as J

    for name in ("encode_jpeg_tensors", "imwrite_jpeg_tensors", "last_encode_batch_report"):
        assert getattr(V, name) is getattr(J, name) and name in V.__all__
    assert V.last_encode_batch_report is not V.last_batch_report
