"""The device PNG encoder without a GPU: the NumPy restatement of the stream (png_ref.py) against zlib, Pillow and this package's
parallel reader; the product's png_core.hpp / png_host.hpp run on the host against the restatement, byte for byte; the code builder;
the size conditions of the format; the C ABI's argument checks; the resource budget of kernels_png.o; the device_png plumbing."""
import ctypes as C
import struct
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

import png_ref as R
import sphere_scene
from vr180_convert_amd import _png, synth

ROOT = Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "host_png" / "png_emul.hip"


class Band(C.Structure):
    _fields_ = [("row0", C.c_uint32), ("row1", C.c_uint32), ("offset", C.c_uint64), ("size", C.c_uint64), ("adler32", C.c_uint32),
                ("stored", C.c_uint32)]


@pytest.fixture(scope="module")
def png_emul(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_png") / "libpng_emul.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-fno-fast-math", "-o", str(out),
                    str(HARNESS)], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(out))
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    lib.png_emul_code_lengths.argtypes = [vp, i32, i32, vp]
    lib.png_emul_bound.argtypes = [i32] * 5
    lib.png_emul_bound.restype = C.c_uint64
    lib.png_emul_deflate.argtypes = [vp, i32, i32, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    return lib


_rng = R._rng
_half_noise = R._half_noise
CASES = R.cases()
PARAMS = [(name, f) for name in CASES for f in ("up", "paeth")]
check_file = R.check_file
_pil = R._pil


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,filter", PARAMS)
def test_restatement_decodes_everywhere(name, filter):
    img, rows = CASES[name]
    check_file(R.encode(img, filter=filter, band_rows=rows), img, filter, rows)


def test_restatement_stored_and_coded_bands():
    _, bands = R.deflate(CASES["noise_full"][0], band_rows=8)
    assert len(bands) == 10 and all(b[5] == 1 for b in bands)  # full-frame noise: every band falls back to stored blocks
    _, bands = R.deflate(_half_noise(), band_rows=8)
    assert [b[5] for b in bands] == [1, 1, 1, 1, 0, 0, 0, 0]
    segs, bands = R.deflate(CASES["noise_big_band"][0], band_rows=50)
    assert bands[0][5] == 1 and bands[0][3] == 50 * 1501 + 10 and segs[0] == 0 and segs[65540] == 0  # two stored blocks
    _, bands = R.deflate(CASES["zero"][0], band_rows=8)
    assert all(b[5] == 0 for b in bands)


def test_restated_filters_equal_the_host_writer_and_pillow():
    img = sphere_scene.render(96)
    host = _png.encode(img, level=1, band_rows=8)
    pos = host.index(b"IDAT")
    (n,) = struct.unpack(">I", host[pos - 4:pos])
    assert zlib.decompress(host[pos + 4:pos + 4 + n]) == R.scanlines(img, "up").tobytes()
    # Paeth: un-filtering the restated scanlines with Pillow's decoder gives the image (checked through a zlib-made file)
    lines = R.scanlines(img, "paeth")
    ihdr = struct.pack(">IIBBBBB", 96, 96, 8, 2, 0, 0, 0)
    png = b"\x89PNG\r\n\x1a\n" + R._chunk(b"IHDR", ihdr) + R._chunk(b"IDAT", zlib.compress(lines.tobytes())) + R._chunk(b"IEND", b"")
    assert np.array_equal(_pil(png), img[..., ::-1])


def test_token_rule_on_a_written_out_case():
    s = np.zeros(600, np.uint8)
    s[0:10] = 5             # literal 5, match 9
    s[10:13] = 9            # literal 9, two more literals (a run of 2 stays literals)
    s[13:18] = 1            # literal, match 4
    s[250:262] = 3          # the run is cut at byte 256: literal + match 5 | literal + match 5
    pos, kind, length = R.tokens(s)
    got = {int(p): (int(k), int(n)) for p, k, n in zip(pos, kind, length)}
    assert got[0] == (1, 0) and got[1] == (2, 9) and 2 not in got
    assert got[10] == got[11] == got[12] == (1, 0)
    assert got[13] == (1, 0) and got[14] == (2, 4)
    assert got[18] == (1, 0) and got[19] == (2, 231)  # zeros up to byte 249
    assert got[250] == (1, 0) and got[251] == (2, 5) and got[256] == (1, 0) and got[257] == (2, 5)
    assert got[262] == (1, 0) and got[263] == (2, 249) and got[512] == (1, 0) and got[513] == (2, 87)


# ---- the product's arithmetic and planner on the host -------------------------------------------------------------------------------
def _emul(lib, img, filter, rows, pitch=None):
    a = np.ascontiguousarray(img if img.ndim == 3 else img[..., None])
    h, w, cn = a.shape
    depth = 2 if a.dtype == np.uint16 else 0
    cap = lib.png_emul_bound(h, w, cn, depth, rows)
    assert cap == R.bound(h, w, cn, a.dtype.itemsize, rows)
    out = np.zeros(cap, np.uint8)
    nb = -(-h // min(rows, h))
    bands = (Band * nb)()
    count, size = C.c_int32(0), C.c_uint64(0)
    rc = lib.png_emul_deflate(a.ctypes.data, h, w, pitch or a.strides[0], cn, depth, R.FILTERS[filter], rows, out.ctypes.data, bands,
                              C.byref(count), C.byref(size), None)
    assert rc == 0 and count.value == nb
    return out[:size.value].tobytes(), [(b.row0, b.row1, b.offset, b.size, b.adler32, b.stored) for b in bands]


@pytest.mark.parametrize("name,filter", PARAMS)
def test_product_host_code_equals_restatement(png_emul, name, filter):
    img, rows = CASES[name]
    got, bands = _emul(png_emul, img, filter, rows)
    want, wbands = R.deflate(img if img.ndim == 3 else img[..., None], filter=filter, band_rows=rows)
    assert bands == wbands
    assert got == want
    a = img if img.ndim == 3 else img[..., None]
    png = _png.assemble(got, [b[:5] for b in bands], width=a.shape[1], height=a.shape[0], channels=a.shape[2],
                        bit_depth=8 * a.dtype.itemsize, filter_type=R.FILTERS[filter])
    assert png == R.encode(img, filter=filter, band_rows=rows)  # (the container: assemble's CRC in parts against zlib's in one piece)


def test_product_host_code_reads_a_pitched_half(png_emul):
    sbs = np.concatenate([sphere_scene.render(64), synth.noise_disc(64, 64)], axis=1)
    right = sbs[:, 64:]
    a = np.ascontiguousarray(right)
    lib = png_emul
    cap = lib.png_emul_bound(64, 64, 3, 0, 8)
    out = np.zeros(cap, np.uint8)
    bands = (Band * 8)()
    count, size = C.c_int32(0), C.c_uint64(0)
    assert lib.png_emul_deflate(right.ctypes.data, 64, 64, sbs.strides[0], 3, 0, 2, 8, out.ctypes.data, bands, C.byref(count),
                                C.byref(size), None) == 0
    assert out[:size.value].tobytes() == R.deflate(a, band_rows=8)[0]


# ---- the code builder ---------------------------------------------------------------------------------------------------------------
def _kraft(lengths):
    return sum(2 ** (15 - int(v)) for v in lengths if v)


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def _histograms():
    rng = _rng(11)
    out = [rng.integers(0, 1000, 286) * (rng.random(286) < 0.6) for _ in range(6)]
    out += [rng.integers(1, 4, 286), (rng.pareto(0.4, 286) * 10).astype(np.int64)]
    one = np.zeros(286, np.int64)
    one[77] = 12
    two = one.copy()
    two[256] = 1
    fib = np.zeros(286, np.int64)
    fib[100:140] = _fib(40)
    return out + [one, two, fib, np.zeros(286, np.int64)]


def test_code_builder(png_emul):
    for k, freq in enumerate(_histograms()):
        freq = np.asarray(freq, np.uint64)
        for limit in (15, 7) if np.count_nonzero(freq) <= 100 else (15,):
            f = freq[:19] if limit == 7 else freq
            if limit == 7 and not f.any():
                f = np.asarray(_fib(19), np.uint64)  # a 19-symbol Fibonacci histogram: the limit of the code-length code is exercised
            got = np.zeros(len(f), np.uint8)
            png_emul.png_emul_code_lengths(np.ascontiguousarray(f).ctypes.data, len(f), limit, got.ctypes.data)
            want = R.code_lengths(f, limit)
            assert got.max() <= limit and _kraft(got) == 1 << 15, (k, limit)
            assert ((got > 0) >= (f > 0)).all()
            cost = int((got.astype(np.int64) * f.astype(np.int64)).sum())
            assert cost <= int((want * f.astype(np.int64)).sum()), (k, limit)
            assert np.array_equal(got, want), (k, limit)
            if np.count_nonzero(f) >= 2:  # the rule's two stages agree on the cost with plain package-merge: both are optimal
                assert cost == int((R.package_merge(f, limit) * f.astype(np.int64)).sum()), (k, limit)
    fib = np.zeros(286, np.int64)
    fib[100:140] = _fib(40)
    assert R.code_lengths(fib, 15).max() == 15 and R.code_lengths(fib, 64).max() == 39  # the unlimited tree is 39 deep


# ---- sizes --------------------------------------------------------------------------------------------------------------------------
def test_size_of_constant_and_incompressible_images():
    # SEG = 256: a constant segment is one literal and one match, a token at most 15 + 5 + 1 bits (under 1.8 % of 256 bytes); the filter
    # byte breaks the run once per 1537-byte row (under 0.4 %); header and tail are under 300 bytes per 12 296-byte band (2.4 %)
    zero = np.zeros((512, 512, 3), np.uint8)
    segs, _ = R.deflate(zero, band_rows=8)
    assert R.SEG >= 256 and len(segs) <= 0.05 * 512 * 1537, len(segs) / (512 * 1537)
    img = synth.noise_disc(512, 512)
    segs, _ = R.deflate(img, band_rows=8)
    assert len(segs) <= R.bound(512, 512, 3, 1, 8)


@pytest.mark.parametrize("name", ["sphere_1024", "pattern_1024", "noise_disc_512"])
def test_size_against_zlib_rle(name):
    """the same filtered scanlines through zlib's own distance-1 coder (level 1, Z_RLE, raw deflate): the stream is at most 1.05 x its"""
    img = {"sphere_1024": lambda: sphere_scene.render(1024), "pattern_1024": lambda: synth.pattern(1024, 1024),
           "noise_disc_512": lambda: synth.noise_disc(512, 512)}[name]()
    segs, _ = R.deflate(img, band_rows=8)
    c = zlib.compressobj(1, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
    ref = len(c.compress(R.scanlines(img, "up").tobytes()) + c.flush())
    print(f"{name}: stream {len(segs)}, zlib Z_RLE {ref}, ratio {len(segs) / ref:.4f}")
    assert len(segs) <= 1.05 * ref, len(segs) / ref


# ---- the library without a device ---------------------------------------------------------------------------------------------------
def test_png_bound_and_argument_validation_without_device(product_lib):
    lib = product_lib
    for h, w, cn, item, rows in [(512, 512, 3, 1, 8), (1, 1, 1, 1, 8), (77, 96, 4, 2, 5), (4096, 8192, 3, 1, 8), (60, 500, 3, 1, 50)]:
        assert lib.v1c_png_bound(h, w, cn, 2 if item == 2 else 0, rows) == R.bound(h, w, cn, item, rows)
    assert lib.v1c_png_bound(8, 8, 2, 0, 8) == 0 and lib.v1c_png_bound(8, 8, 3, 5, 8) == 0 and lib.v1c_png_bound(8, 8, 3, 0, 0) == 0
    buf = np.zeros(1 << 16, np.uint8)  # stands in for the device pointer: validation fails before any device call
    out = np.zeros(1 << 16, np.uint8)
    bands = (Band * 64)()
    count, size = C.c_int32(0), C.c_uint64(0)

    def call(img=buf.ctypes.data, h=64, w=64, pitch=192, cn=3, depth=0, filter=2, rows=8, dst=out.ctypes.data, cap=1 << 16, b=bands):
        return lib.v1c_png_deflate(0, None, img, h, w, pitch, cn, depth, filter, rows, dst, cap, b, C.byref(count), C.byref(size))

    def err():
        return lib.v1c_last_error().decode()

    assert call(cn=2) == -1 and "cn" in err()
    assert call(depth=5) == -1 and "depth" in err()
    assert call(filter=1) == -1 and "filter" in err()
    assert call(img=None) == -1 and "NULL" in err()
    assert call(dst=None) == -1 and "NULL" in err()
    assert call(b=None) == -1 and "NULL" in err()
    assert call(cap=1000) == -1 and "capacity" in err()
    assert call(pitch=191) == -1 and "pitch" in err()
    assert call(rows=0) == -1 and call(h=0) == -1 and call(w=1 << 21) == -1
    assert call(depth=2, pitch=385, cap=1 << 16) == -1 and "even" in err()
    assert call(depth=2, pitch=384, img=buf.ctypes.data + 1) == -1 and "even" in err()


def test_kernels_png_use_no_scratch_and_spill_nothing(tmp_path, product_lib):
    from test_resource_budget import kernel_metadata

    obj = ROOT / "vr180_convert_amd" / "csrc" / "kernels_png.o"
    assert obj.exists(), "kernels_png.o is built by __graft_entry__.build() / make"
    kernels = kernel_metadata(tmp_path, obj)
    assert len(kernels) >= 6 and all("k_png_" in k[".name"] for k in kernels)
    bad = [(k[".name"], k[".private_segment_fixed_size"], k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for k in kernels
           if k[".private_segment_fixed_size"] or k[".sgpr_spill_count"] or k[".vgpr_spill_count"]]
    assert not bad, bad
    assert all(k[".wavefront_size"] == 64 for k in kernels)


def test_crc32_combine():
    rng = _rng(5)
    for n1, n2 in [(0, 5), (5, 0), (1, 1), (1000, 77), (70000, 1 << 20)]:
        a, b = rng.bytes(n1), rng.bytes(n2)
        assert _png.crc32_combine(zlib.crc32(a), zlib.crc32(b), n2) == zlib.crc32(a + b)
    big = rng.bytes(9 << 20)
    assert _png._crc32_parallel([b"IDAT", big[:5], big, b""], 4) == zlib.crc32(b"IDAT" + big[:5] + big)


# ---- device_png plumbing --------------------------------------------------------------------------------------------------------------
def test_eligibility_and_type_checks():
    import torch

    from vr180_convert_amd import png_device as P

    host = torch.zeros((4, 4, 3), dtype=torch.uint8)
    assert not P.eligible("a.png", host) and not P.eligible("a.png", np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(TypeError):
        P.encode_png_tensor(host)
    with pytest.raises(ValueError):
        P.deflate_tensor(host, filter="sub")
    assert P.default_band_rows(4096, 8192 * 3 + 1) == 8 and P.default_band_rows(3, 10) == 3 and P.default_band_rows(100, 1 << 20) == 1


class _FakeCuda:
    """stands in for a CUDA tensor where only the routing is under test"""

    def __init__(self, a):
        import torch

        self.a, self.dtype, self.is_cuda = a, {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16,
                                                np.dtype(np.float32): torch.float32}[a.dtype], True

    def cpu(self):
        import torch

        return torch.from_numpy(self.a)


def test_device_png_plumbing_reaches_imwrite_tensor_only_for_eligible_results(tmp_path, monkeypatch):
    import torch

    from vr180_convert_amd import _io, png_device, remapper

    dev_writes, host_writes = [], []
    monkeypatch.setattr(png_device, "eligible", lambda p, r: str(p).lower().endswith(".png") and getattr(r, "is_cuda", False)
                        and r.dtype in (torch.uint8, torch.uint16))
    monkeypatch.setattr(png_device, "imwrite_tensor", lambda p, t, **k: dev_writes.append(Path(p).name))
    monkeypatch.setattr(_io, "imwrite", lambda p, a: host_writes.append(Path(p).name) or True)
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
        dev_writes.clear(), host_writes.clear()
        remapper.apply_lr(None, left_path=img, right_path=img, out_path=tmp_path / name, size_output=(4, 4), **kw)
        return list(dev_writes), list(host_writes)

    assert lr("a.png", device_png=True) == (["a.png"], [])
    assert lr("a.PNG", device_png=True) == (["a.PNG"], [])
    assert lr("a.png") == ([], ["a.png"])                       # off by default
    assert lr("a.png", device_png=False) == ([], ["a.png"])
    assert lr("a.npy", device_png=True) == ([], ["a.npy"])
    assert lr("a.jpg", device_png=True) == ([], ["a.jpg"])
    kind["v"] = "u16"
    assert lr("a.png", device_png=True) == (["a.png"], [])
    kind["v"] = "f32"
    assert lr("a.png", device_png=True) == ([], ["a.png"])      # float32 results are saturated by the host writer
    kind["v"] = "u8"
    monkeypatch.setattr(remapper, "anaglyph_tensors", lambda l, r: _FakeCuda(np.zeros((4, 4, 3), np.float64).astype(np.float32)))
    monkeypatch.setattr(_io, "draw_anaglyph_labels", lambda a: a)
    results["u8"] = _FakeSbs(np.zeros((4, 8, 3), np.uint8))
    assert lr("a.png", device_png=True, merge=True) == ([], ["a.png"])  # the anaglyph is float64 on the host


class _FakeSbs(_FakeCuda):
    def __getitem__(self, key):
        return self


def test_cli_flag_reaches_apply_and_apply_lr(tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from vr180_convert_amd import _io, cli, remapper

    seen = []
    monkeypatch.setattr(remapper, "apply_lr", lambda *a, **k: seen.append(("lr", k.get("device_png"))))
    monkeypatch.setattr(remapper, "apply", lambda *a, **k: seen.append(("s", k.get("device_png"))))
    img = tmp_path / "a.png"
    _io.imwrite(img, synth.pattern(64, 64))
    run = CliRunner().invoke
    base = ["--radius", "max", "--size", "32x32"]
    assert run(cli.app, ["lr", str(img), str(img), *base, "--device-png", "--out-path", str(tmp_path / "o.png")]).exit_code == 0
    assert run(cli.app, ["lr", str(img), str(img), *base, "--out-path", str(tmp_path / "o.png")]).exit_code == 0
    assert run(cli.app, ["s", str(img), *base, "--device-png", "--out-path", str(tmp_path / "o.png")]).exit_code == 0
    assert run(cli.app, ["s", str(img), *base, "--out-path", str(tmp_path / "o.png")]).exit_code == 0
    assert seen == [("lr", True), ("lr", None), ("s", True), ("s", None)]


# ---- the boundary images the GPU half runs (tests/png_cases.py): generators and restatement proven on the host first --------------
import png_cases as PC  # noqa: E402

EDGE_PARAMS = [(name, f) for name in PC.shared_cases() for f in ("up", "paeth")]


def test_from_filtered_gives_the_filtered_bytes():
    rng = _rng(21)
    f = PC.run_plane(rng, 9, 300)
    assert np.array_equal(R.scanlines(PC.from_filtered(f), "up"), f)
    f = PC.fibonacci_row(rng, 21)
    assert f.shape == (1, 28656) and np.array_equal(R.scanlines(PC.from_filtered(f), "up"), f)
    assert sorted(np.bincount(f.reshape(-1))[np.bincount(f.reshape(-1)) > 0].tolist()) == sorted(PC._fib(21))


def test_edge_cases_sit_on_the_boundaries_they_are_for():
    """What the list must contain (both filters over all of it), and the band sizes that name the kernels' boundaries."""
    cases = PC.shared_cases()
    stats = {(n, f): PC.band_stats(img, f, rows) for n, (img, rows) in cases.items() for f in ("up", "paeth")}
    coded = [b for s in stats.values() for b in s if not b["stored"]]
    assert any(b["max_len"] == 15 for b in coded)                      # a code with a 15-bit length
    assert any(b["depth"] > 15 for b in coded)                         # package-merge engages
    lengths = set().union(*(b["matches"] for b in coded))
    assert min(lengths) == 4 and max(lengths) == 255
    for lo, hi in ((4, 10), (11, 130), (131, 255)):
        assert any(lo <= v <= hi for v in lengths), (lo, hi)
    assert {62, 63, 64, 65, 66, 127, 128, 129, 250, 255} <= lengths  # runs of 63 ... 67, 128 ... 130, 251, 256 and more bytes: across the lane steps
    assert any(len({b["stored"] for b in s}) == 2 for s in stats.values())  # stored and coded bands in one file
    size = {n: [b["nbytes"] for b in stats[(n, "up")]] for n in cases}
    assert size["runs_stride256_8rows"] == [2048] * 3 and size["runs_stride257_1row"] == [257] * 7
    assert size["runs_16384"] == [64 * 256] and size["runs_16448"] == [65 * 256 - 192]
    assert size["runs_65536"] == [256 * 256] and size["runs_65792"] == [257 * 256 - 0] and size["runs_65792_two_values"][0] == 65792
    assert size["fib21_one_row"] == [28656] and size["fib24_stride602"] == [64 * 602] * 2
    for n in (65535, 65536, 65537, 131070, 131071):
        assert size[f"noise_{n}"] == [n] and all(b["stored"] for b in stats[(f"noise_{n}", "up")] + stats[(f"noise_{n}", "paeth")])
    assert [b["stored"] for b in stats[("noise_then_runs", "up")]] == [True, False]
    assert {cases[n][0].dtype.itemsize * cases[n][0].shape[2] for n in cases} == {1, 2, 3, 4, 6, 8}  # every bytes-per-pixel the kernels have
    for n in ("runs_gray16_16448", "runs_bgra16_65792", "runs_bgra_65792", "runs_bgr_16384"):
        assert size[n][0] in (16384, 16448, 65792) and not stats[(n, "up")][0]["stored"]


@pytest.mark.parametrize("name,filter", EDGE_PARAMS)
def test_edge_cases_product_host_code_equals_restatement(png_emul, name, filter):
    img, rows = PC.shared_cases()[name]
    want, wbands, wfile = PC.reference(name, filter)
    got, bands = _emul(png_emul, img, filter, rows)
    assert bands == wbands  # (row0, row1, offset, size, adler32, stored) of every band
    assert got == want
    check_file(wfile, img, filter, rows)
    png = _png.assemble(got, [b[:5] for b in bands], width=img.shape[1], height=img.shape[0], channels=img.shape[2],
                        bit_depth=8 * img.dtype.itemsize, filter_type=R.FILTERS[filter])
    assert png == wfile
