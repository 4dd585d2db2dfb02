"""The device JPEG encoder without a GPU: the NumPy restatement of the file (jpg_ref.py) against Pillow; the product's jpeg_core.hpp /
jpeg_host.hpp run on the host against the restatement, byte for byte; the case list the GPU half shares; the size bound; the C ABI's
argument checks; the resource budget of kernels_jpeg.o; the device_jpeg plumbing."""
import ctypes as C
import io
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jpg_cases as PC
import jpg_ref as R
import sphere_scene

ROOT = Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "host_jpeg" / "jpeg_emul.hip"
CASES = PC.shared_cases()

# What the restatement may lose against Pillow's own encoder (libjpeg: the same tables, DCT and quantiser) at the same quality and
# subsampling, both decoded by Pillow: the measured gaps below, rounded up to the next 0.1 dB.  The gap comes from the chroma
# rounding -- the contract rounds the colour conversion and the 2 x 2 mean half up, libjpeg rounds the conversion to nearest and
# alternates the mean's bias -- and is nothing in 4:4:4 luminance.  Measured on the CPU (dB, Pillow minus restatement):
#   docs image 2048 x 2048   420/50: 0.014   420/95: 0.034   444/50: 0.000   444/95: 0.000
#   sphere_scene 512         420/50: 0.000   420/95: 0.000   444/50: 0.000   444/95: 0.000   (a grey scene: no chroma to round)
PSNR_MARGIN_DB = 0.1


@pytest.fixture(scope="module")
def jpeg_emul(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_jpeg") / "libjpeg_emul.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-fno-fast-math", "-o", str(out),
                    str(HARNESS)], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(out))
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    lib.jpeg_emul_bound.argtypes = [i32] * 5
    lib.jpeg_emul_bound.restype = C.c_uint64
    lib.jpeg_emul_encode.argtypes = [vp, i32, i32, i64, i32, i32, i32, i32, vp, vp, vp, C.c_uint64, vp]
    return lib


def _pillow(img, quality, subsampling):
    from PIL import Image

    a = img[..., 0] if img.shape[2] == 1 else img[..., 2::-1]
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(a)).save(b, "JPEG", quality=quality, subsampling=R.SUBSAMPLINGS[subsampling])
    return b.getvalue()


def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_pillow_opens_every_file(name):
    from PIL import Image

    c = CASES[name]
    data = PC.reference(name)[2]
    im = Image.open(io.BytesIO(data))
    assert im.size == (c.w, c.h) and im.mode == ("L" if c.cn == 1 else "RGB")
    im.load()
    own = Image.open(io.BytesIO(_pillow(np.ascontiguousarray(c.image()), c.quality, c.subsampling)))
    assert im.quantization == own.quantization
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9" and data[6:11] == b"JFIF\x00"
    # decodes to the image as well as Pillow's own file does (small images: a loose check that nothing is misplaced)
    got, ref = np.asarray(im).astype(np.int64), np.asarray(own).astype(np.int64)
    src = c.image()[..., 0] if c.cn == 1 else c.image()[..., 2::-1]
    assert np.abs(got - src).mean() <= np.abs(ref - src).mean() + 1.0


def test_vectorised_coder_equals_the_plain_one():
    for name in ("size_17x17_420", "zero_runs", "only_63", "swing_q100", "noise_q100_444", "restart2_420", "quality_1"):
        c = CASES[name]
        g = R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart)
        zz = PC.reference(name)[0]
        blk, bits, length = R.tokens(zz, g)
        diff = R.dc_differences(zz, g)
        for b in range(g.nblocks):
            tab = min(int(g.comp[b % g.bpm]), 1)
            want = R.encode_block_scalar(zz[b], int(zz[b, 0]) - int(diff[b]), tab)
            m = blk == b
            # (the vectorised coder joins ZRLs to the coefficient behind them: compare the concatenated bits)
            cat = lambda toks: "".join(format(v, f"0{n}b") for v, n in toks if n)  # noqa: E731
            assert cat(zip(bits[m].tolist(), length[m].tolist())) == cat(want), (name, b)


def test_dc_prediction_resets_at_every_interval():
    c = CASES["restart2_420"]
    g = R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart)
    zz = PC.reference("restart2_420")[0]
    diff = R.dc_differences(zz, g)
    first = np.arange(g.nblocks) % (g.bpm * g.restart)
    assert np.array_equal(diff[first == 0], zz[first == 0, 0])       # Y of an interval's first MCU
    assert np.array_equal(diff[first == 4], zz[first == 4, 0])       # Cb
    assert np.array_equal(diff[first == 1], zz[first == 1, 0] - zz[first == 0, 0].astype(np.int64))


@pytest.mark.parametrize("source", ["docs", "sphere"])
def test_quality_against_pillow(source):
    from PIL import Image

    if source == "docs":
        img = np.ascontiguousarray(np.asarray(Image.open(ROOT / "tests" / "golden" / "ref_docs" / "test.jpg").convert("RGB"))[..., ::-1])
    else:
        img = sphere_scene.render(512)
    for sub in ("420", "444"):
        for q in (50, 95):
            mine = _psnr(R.decode(R.encode(img, q, sub)), img)
            theirs = _psnr(R.decode(_pillow(img, q, sub)), img)
            print(f"{source} {sub} q{q}: restatement {mine:.3f} dB, Pillow {theirs:.3f} dB, gap {theirs - mine:.3f}")
            assert mine >= theirs - PSNR_MARGIN_DB, (source, sub, q, mine, theirs)


# ---- the case list ------------------------------------------------------------------------------------------------------------------
def _stats(name):
    c = CASES[name]
    g = R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart)
    zz = PC.reference(name)[0]
    return c, g, zz


def _zero_runs(zz):
    runs = set()
    for b in zz:
        nz = np.nonzero(b[1:])[0] + 1
        runs |= set((nz - np.concatenate([[0], nz[:-1]]) - 1).tolist())
    return runs


def test_case_list_sits_on_the_boundaries_it_is_for():
    for h, w in [(1, 1), (7, 9), (8, 8), (16, 16), (17, 17), (15, 33), (31, 16)]:
        for kind in ("420", "444", "gray"):
            c = CASES[f"size_{h}x{w}_{kind}"]
            assert (c.h, c.w) == (h, w)
    geoms = {n: R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart) for n, c in CASES.items()}
    # partial MCUs in either axis, for both MCU sizes
    for m in (8, 16):
        assert any(g.m == m and g.w % m for g in geoms.values()) and any(g.m == m and g.h % m and not g.w % m for g in geoms.values())
        assert any(g.m == m and g.w % m and g.h % m for g in geoms.values()) and any(g.m == m and g.w < m and g.h < m for g in geoms.values())
    assert any(g.restart % g.mcux and g.nint > 2 for g in geoms.values())                 # an interval ends mid-row
    assert any(g.restart == 1 and g.nmcu > 1 for g in geoms.values())
    assert any(g.restart == g.nmcu and g.nmcu > 1 for g in geoms.values()) and any(g.restart > g.nmcu > 1 for g in geoms.values())
    assert any(g.restart == 65535 for g in geoms.values())
    assert sum(g.nint >= 17 for g in geoms.values()) >= 2 and geoms["restart1_444"].nint == 45  # RSTm wraps twice (and five times)
    # the flat image: EOB only, every DC difference 0
    c, g, zz = _stats("flat")
    assert not zz.any() and set(PC.reference("flat")[1].tolist()) == {2 + 4, 2 + 2}
    # the only AC coefficient at zigzag 63; zero runs of 15, 16, 17 and 33; blocks that end without EOB
    c, g, zz = _stats("only_63")
    assert [np.nonzero(b)[0].tolist() for b in zz] == [[63], [63], [0, 63]] and _zero_runs(zz) == {62}
    c, g, zz = _stats("zero_runs")
    assert {15, 16, 17, 33} <= _zero_runs(zz) and zz[3, 63] != 0 and zz[0, 63] == 0
    # full swing: a DC difference of category 11 and an AC coefficient of category 10
    c, g, zz = _stats("swing_q100")
    assert c.quality == 100 and int(np.abs(R.dc_differences(zz, g)).max()).bit_length() == 11
    assert int(np.abs(zz[:, 1:]).max()).bit_length() == 10
    # noise at quality 100: many stuffed bytes
    for n in ("noise_q100_444", "noise_q100_420", "noise_gray_q100_r1"):
        raw = b"".join(b for _, b in PC.intervals(n))
        assert CASES[n].quality == 100 and raw.count(b"\xff") >= 20, (n, raw.count(b"\xff"))
    # an interval of a multiple of 8 bits (no pad); an interval whose padded last byte is 0xFF (stuffed too)
    iv = PC.intervals("noise_gray_q100_r1")
    assert any(n % 8 == 0 for n, _ in iv) and any(n % 8 and b[-1] == 0xFF for n, b in iv)
    data = PC.reference("noise_gray_q100_r1")[2]
    assert any(data.find(b"\xff\x00\xff" + bytes([0xD0 + m])) > 0 for m in range(8))
    assert {c.quality for c in CASES.values()} >= {1, 49, 50, 95, 100}
    assert {c.cn for c in CASES.values()} == {1, 3, 4} and {c.subsampling for c in CASES.values()} == {"420", "444"}
    assert any(c.pitch > c.w * c.cn and c.offset % 2 == 0 for c in CASES.values())        # the right half of a wider image
    assert {c.cn for c in CASES.values() if c.offset % 2} == {1, 3, 4}                    # behind an odd byte offset
    assert CASES["right_half"].offset == 64 * 3 and CASES["right_half"].pitch == 128 * 3


def test_every_case_is_quick():
    import time

    t = time.perf_counter()
    for name in CASES:
        PC.reference(name)
    assert time.perf_counter() - t < 0.5 * len(CASES)


# ---- the product's arithmetic on the host -------------------------------------------------------------------------------------------
def _emul(lib, c):
    g = R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart)
    sub = R.SUBSAMPLINGS[c.subsampling]
    cap = lib.jpeg_emul_bound(c.h, c.w, c.cn, sub, c.restart)
    assert cap == R.bound(c.h, c.w, c.cn, c.subsampling, c.restart)
    coef = np.zeros((g.nblocks, 64), np.int16)
    bits = np.zeros(g.nblocks, np.uint32)
    out = np.zeros(cap + 1024, np.uint8)
    size = C.c_uint64(0)
    rc = lib.jpeg_emul_encode(c.base.ctypes.data + c.offset, c.h, c.w, c.pitch, c.cn, c.quality, sub, c.restart, coef.ctypes.data,
                              bits.ctypes.data, out.ctypes.data, out.size, C.byref(size))
    assert rc == 0
    return coef, bits, out[:size.value].tobytes()


@pytest.mark.parametrize("name", list(CASES))
def test_product_host_code_equals_restatement(jpeg_emul, name):
    coef, bits, data = _emul(jpeg_emul, CASES[name])
    zz, wbits, wdata = PC.reference(name)
    assert np.array_equal(coef, zz)
    assert np.array_equal(bits, wbits)
    assert data == wdata
    assert bits.max() <= R.MAX_BLOCK_BITS


def test_zigzag_rule(jpeg_emul):
    assert [jpeg_emul.jpeg_emul_zigzag(int(n)) for n in R.ZIGZAG] == list(range(64))


# ---- the library without a device ---------------------------------------------------------------------------------------------------
def test_bound_is_never_exceeded_and_arguments_are_validated_without_device(product_lib):
    lib = product_lib
    lib.v1c_jpeg_bound.restype = C.c_uint64
    for name, c in CASES.items():
        cap = lib.v1c_jpeg_bound(c.h, c.w, c.cn, R.SUBSAMPLINGS[c.subsampling], c.restart)
        assert cap == R.bound(c.h, c.w, c.cn, c.subsampling, c.restart)
        head = len(R.headers(R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart), c.quality))
        assert len(PC.reference(name)[2]) - head - 2 <= cap, name
    assert lib.v1c_jpeg_bound(4096, 8192, 3, 2, 512) == R.bound(4096, 8192, 3, "420", 512)
    for bad in [(8, 8, 2, 2, 1), (8, 8, 3, 1, 1), (8, 8, 3, 2, 0), (8, 8, 3, 2, 65536), (0, 8, 3, 2, 1), (8, 65536, 3, 2, 1)]:
        assert lib.v1c_jpeg_bound(*bad) == 0, bad
    assert lib.v1c_jpeg_bound(65535, 65535, 3, 0, 65535) > 0
    # the header call
    lib.v1c_jpeg_header.restype = C.c_int64
    lib.v1c_jpeg_header.argtypes = [C.c_int] * 6 + [C.c_void_p, C.c_uint64]
    head = np.zeros(1024, np.uint8)
    for name in ("size_17x17_420", "size_7x9_gray", "bgra_444", "restart_max"):
        c = CASES[name]
        n = lib.v1c_jpeg_header(c.h, c.w, c.cn, c.quality, R.SUBSAMPLINGS[c.subsampling], c.restart, head.ctypes.data, 1024)
        assert head[:n].tobytes() == R.headers(R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart), c.quality)
    assert lib.v1c_jpeg_header(8, 8, 3, 95, 2, 1, head.ctypes.data, 100) == -1 and lib.v1c_jpeg_header(8, 8, 3, 0, 2, 1, head.ctypes.data, 1024) == -1
    assert lib.v1c_jpeg_header(8, 8, 3, 95, 2, 1, None, 1024) == -1

    lib.v1c_jpeg_encode.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.c_uint64, C.c_void_p]
    buf = np.zeros(1 << 16, np.uint8)  # stands in for the device pointer: validation fails before any device call
    out = np.zeros(1 << 20, np.uint8)
    size = C.c_uint64(0)

    def call(img=buf.ctypes.data, h=64, w=64, pitch=192, cn=3, quality=95, sub=2, restart=4, dst=out.ctypes.data, cap=1 << 20, sz=C.byref(size)):
        return lib.v1c_jpeg_encode(0, None, img, h, w, pitch, cn, quality, sub, restart, dst, cap, sz)

    def err():
        return lib.v1c_last_error().decode()

    assert lib.v1c_jpeg_bound(64, 64, 3, 2, 4) <= 1 << 20
    assert call(cn=2) == -1 and "cn" in err()
    assert call(quality=0) == -1 and "quality" in err() and call(quality=101) == -1
    assert call(sub=1) == -1 and "subsampling" in err()
    assert call(restart=0) == -1 and "restart" in err() and call(restart=65536) == -1
    assert call(h=0) == -1 and call(w=0) == -1 and call(h=65536) == -1 and "65535" in err() and call(w=65536, pitch=1 << 20) == -1
    assert call(img=None) == -1 and "NULL" in err()
    assert call(dst=None) == -1 and "NULL" in err()
    assert call(sz=None) == -1 and "NULL" in err()
    assert call(cap=1000) == -1 and "capacity" in err()
    assert call(cap=lib.v1c_jpeg_bound(64, 64, 3, 2, 4) - 1) == -1 and "capacity" in err()
    assert call(pitch=191) == -1 and "pitch" in err()


def test_kernels_jpeg_use_no_scratch_and_spill_nothing(tmp_path, product_lib):
    from test_resource_budget import kernel_metadata

    obj = ROOT / "vr180_convert_amd" / "csrc" / "kernels_jpeg.o"
    assert obj.exists(), "kernels_jpeg.o is built by __graft_entry__.build() / make"
    kernels = kernel_metadata(tmp_path, obj)
    assert len(kernels) >= 9 and all("k_jpeg_" in k[".name"] for k in kernels)
    bad = [(k[".name"], k[".private_segment_fixed_size"], k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for k in kernels
           if k[".private_segment_fixed_size"] or k[".sgpr_spill_count"] or k[".vgpr_spill_count"]]
    assert not bad, bad
    assert all(k[".wavefront_size"] == 64 for k in kernels)


# ---- device_jpeg plumbing -----------------------------------------------------------------------------------------------------------
def test_eligibility_and_type_checks():
    import torch

    import vr180_convert_amd as V
    from vr180_convert_amd import jpeg_device as J

    assert V.encode_jpeg_tensor is J.encode_jpeg_tensor and V.imwrite_jpeg_tensor is J.imwrite_jpeg_tensor
    host = torch.zeros((4, 4, 3), dtype=torch.uint8)
    assert not J.eligible("a.jpg", host) and not J.eligible("a.jpg", np.zeros((4, 4, 3), np.uint8))
    dev = _FakeCuda(np.zeros((4, 4, 3), np.uint8))
    real = J.torch.Tensor
    try:
        J.torch.Tensor = _FakeCuda  # (only the isinstance test of `eligible` sees it)
        assert J.eligible("a.jpg", dev) and J.eligible(Path("b/a.JPEG"), dev) and not J.eligible("a.png", dev) and not J.eligible(None, dev)
        assert not J.eligible("a.jpg", _FakeCuda(np.zeros((4, 4, 3), np.uint16))) and not J.eligible("a.jpg", _FakeCuda(np.zeros((4, 4, 3), np.float32)))
    finally:
        J.torch.Tensor = real
    with pytest.raises(TypeError):
        J.encode_jpeg_tensor(host)
    with pytest.raises(ValueError):
        J.encode_jpeg_tensor(host, subsampling="422")
    with pytest.raises(ValueError):
        J.encode_jpeg_tensor(host, quality=0)
    assert J.default_restart_mcus(4096, 8192, 3) == 512 and J.default_restart_mcus(4096, 8192, 3, "444") == 1024
    assert J.default_restart_mcus(5, 5, 1) == 1 and J.default_restart_mcus(4096, 8192, 1, "420") == 1024
    for h, w, cn, sub in [(4096, 8192, 3, "420"), (17, 33, 1, "420"), (17, 33, 4, "444")]:
        assert J.default_restart_mcus(h, w, cn, sub) == R.default_restart_mcus(h, w, cn, sub)
    assert J.SUBSAMPLINGS == R.SUBSAMPLINGS


class _FakeCuda:
    """stands in for a CUDA tensor where only the routing is under test"""

    def __init__(self, a):
        import torch

        self.a, self.dtype, self.is_cuda = a, {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16,
                                                np.dtype(np.float32): torch.float32}[a.dtype], True

    def cpu(self):
        import torch

        return torch.from_numpy(self.a)

    def __getitem__(self, key):
        return self


def test_device_jpeg_plumbing_reaches_the_device_writer_only_for_eligible_results(tmp_path, monkeypatch):
    import torch

    from vr180_convert_amd import _io, jpeg_device, png_device, remapper

    jpg_writes, png_writes, host_writes = [], [], []
    monkeypatch.setattr(jpeg_device, "eligible", lambda p, r: str(p).lower().endswith((".jpg", ".jpeg")) and getattr(r, "is_cuda", False)
                        and r.dtype == torch.uint8)
    monkeypatch.setattr(png_device, "eligible", lambda p, r: str(p).lower().endswith(".png") and getattr(r, "is_cuda", False)
                        and r.dtype in (torch.uint8, torch.uint16))
    monkeypatch.setattr(jpeg_device, "imwrite_jpeg_tensor", lambda p, t, **k: jpg_writes.append(Path(p).name))
    monkeypatch.setattr(png_device, "imwrite_tensor", lambda p, t, **k: png_writes.append(Path(p).name))
    monkeypatch.setattr(_io, "imwrite", lambda p, a: host_writes.append(Path(p).name) or True)
    monkeypatch.setattr(_io, "imwrite_many", lambda ps, ims: host_writes.extend(Path(p).name for p in ps))
    monkeypatch.setattr(_io, "imread_many", lambda paths: list(paths))
    monkeypatch.setattr(remapper, "_to_device", lambda im, dev: im)
    monkeypatch.setattr(remapper, "_device", lambda device=None: torch.device("cpu"))
    monkeypatch.setattr(remapper, "_radius_for_pair", lambda *a: 1.0)
    results = {"u8": _FakeCuda(np.zeros((4, 8, 3), np.uint8)), "u16": _FakeCuda(np.zeros((4, 8, 3), np.uint16)),
               "f32": _FakeCuda(np.zeros((4, 8, 3), np.float32))}
    kind = {"v": "u8"}
    monkeypatch.setattr(remapper, "apply_lr_tensors", lambda *a, **k: results[kind["v"]])
    img = np.zeros((4, 4, 3), np.uint8)

    def lr(name, **kw):
        jpg_writes.clear(), png_writes.clear(), host_writes.clear()
        remapper.apply_lr(None, left_path=img, right_path=img, out_path=tmp_path / name, size_output=(4, 4), **kw)
        return list(jpg_writes), list(png_writes), list(host_writes)

    assert lr("a.jpg", device_jpeg=True) == (["a.jpg"], [], [])
    assert lr("a.JPEG", device_jpeg=True) == (["a.JPEG"], [], [])
    assert lr("a.jpg") == ([], [], ["a.jpg"])                              # off by default
    assert lr("a.jpg", device_jpeg=False) == ([], [], ["a.jpg"])
    assert lr("a.jpg", device_png=True) == ([], [], ["a.jpg"])             # as before this option
    assert lr("a.png", device_jpeg=True) == ([], [], ["a.png"])
    assert lr("a.png", device_jpeg=True, device_png=True) == ([], ["a.png"], [])
    assert lr("a.jpg", device_jpeg=True, device_png=True) == (["a.jpg"], [], [])
    assert lr("a.npy", device_jpeg=True) == ([], [], ["a.npy"])
    for k in ("u16", "f32"):
        kind["v"] = k
        assert lr("a.jpg", device_jpeg=True) == ([], [], ["a.jpg"])        # wide results are saturated by the host writer
    kind["v"] = "u8"
    monkeypatch.setattr(remapper, "anaglyph_tensors", lambda l, r: _FakeCuda(np.zeros((4, 4, 3), np.float32)))
    monkeypatch.setattr(_io, "draw_anaglyph_labels", lambda a: a)
    assert lr("a.jpg", device_jpeg=True, merge=True) == ([], [], ["a.jpg"])  # the anaglyph is made on the host

    # apply: every result by itself
    monkeypatch.setattr(remapper, "get_radius_smart", lambda r, ims: 1.0)
    monkeypatch.setattr(remapper, "remap_tensors", lambda *a, **k: None)
    monkeypatch.setattr(remapper.torch, "empty", lambda shape, dtype=None, device=None: _FakeCuda(np.zeros(shape, np.uint8)))
    srcs = [_FakeCuda(np.zeros((4, 4, 3), np.uint8)) for _ in range(3)]
    for s_ in srcs:
        s_.shape, s_.device = (4, 4, 3), torch.device("cpu")
    monkeypatch.setattr(remapper, "_to_device", lambda im, dev: im)

    def s(names, **kw):
        jpg_writes.clear(), png_writes.clear(), host_writes.clear()
        remapper.apply(None, in_paths=srcs, out_paths=[tmp_path / n for n in names], size_output=(4, 4), **kw)
        return list(jpg_writes), list(png_writes), list(host_writes)

    assert s(["a.jpg", "b.png", "c.npy"], device_jpeg=True) == (["a.jpg"], [], ["b.png", "c.npy"])
    assert s(["a.jpg", "b.png", "c.npy"], device_jpeg=True, device_png=True) == (["a.jpg"], ["b.png"], ["c.npy"])
    assert s(["a.jpg", "b.png", "c.npy"]) == ([], [], ["a.jpg", "b.png", "c.npy"])


def test_cli_flag_reaches_apply_and_apply_lr(tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from vr180_convert_amd import _io, cli, remapper, synth

    seen = []
    monkeypatch.setattr(remapper, "apply_lr", lambda *a, **k: seen.append(("lr", k.get("device_jpeg"), k.get("device_png"))))
    monkeypatch.setattr(remapper, "apply", lambda *a, **k: seen.append(("s", k.get("device_jpeg"), k.get("device_png"))))
    img = tmp_path / "a.png"
    _io.imwrite(img, synth.pattern(64, 64))
    run = CliRunner().invoke
    base = ["--radius", "max", "--size", "32x32"]
    assert run(cli.app, ["lr", str(img), str(img), *base, "--device-jpeg", "--out-path", str(tmp_path / "o.jpg")]).exit_code == 0
    assert run(cli.app, ["lr", str(img), str(img), *base, "--out-path", str(tmp_path / "o.jpg")]).exit_code == 0
    assert run(cli.app, ["s", str(img), *base, "--device-jpeg", "--device-png", "--out-path", str(tmp_path / "o.jpg")]).exit_code == 0
    assert run(cli.app, ["s", str(img), *base, "--out-path", str(tmp_path / "o.jpg")]).exit_code == 0
    assert seen == [("lr", True, None), ("lr", None, None), ("s", True, True), ("s", None, None)]
