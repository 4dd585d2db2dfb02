"""The optimised Huffman tables of the device JPEG encoder without a GPU: the restatement (jpg_opt_ref.py) against Pillow and against
the table rules; the product's symbol walk and table builder (jpeg_core.hpp, jpeg_opt_core.hpp) run on the host against the
restatement, byte for byte; the size bound; the host-only header entry; the resource notes of kernels_jpeg_opt.o; the optimize
plumbing."""
import ctypes as C
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import jpg_opt_cases as K
import jpg_opt_ref as O
import jpg_ref as R

ROOT = Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "host_jpeg_opt" / "jpeg_opt_emul.hip"
CASES = K.shared_cases()
DHT_MAX = 4 * (1 + 16 + 256)


@pytest.fixture(scope="module")
def opt_emul(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_jpeg_opt") / "libjpeg_opt_emul.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-fno-fast-math", "-o", str(out),
                    str(HARNESS)], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(out))
    vp, i32 = C.c_void_p, C.c_int
    lib.jpeg_opt_emul_encode.argtypes = [vp, i32, i32, C.c_int64, i32, i32, i32, i32, vp, vp, vp, C.c_uint64, vp]
    return lib


def _emul(lib, c):
    hist = np.zeros((4, 256), np.uint64)
    codes = np.zeros(32 + 512, np.uint32)
    out = np.zeros(R.bound(c.h, c.w, c.cn, c.subsampling, c.restart) + 4096, np.uint8)
    size = C.c_uint64(0)
    rc = lib.jpeg_opt_emul_encode(c.base.ctypes.data + c.offset, c.h, c.w, c.pitch, c.cn, c.quality, R.SUBSAMPLINGS[c.subsampling], c.restart,
                                  hist.ctypes.data, codes.ctypes.data, out.ctypes.data, out.size, C.byref(size))
    assert rc == 0, rc
    return hist, codes, out[:size.value].tobytes()


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_pillow_decodes_the_optimised_file_to_the_standard_file_s_pixels(name):
    c = CASES[name]
    _, _, data, std, _ = K.reference(name)
    a, b = R.decode(data), R.decode(std)
    assert a.shape[:2] == (c.h, c.w) and np.array_equal(a, b)   # the coefficients are the same: no tolerance
    assert data != std


@pytest.mark.parametrize("name", list(CASES))
def test_every_table_follows_the_rules(name):
    hist, specs, data, _, _ = K.reference(name)
    assert [(tc, bits, vals) for tc, (bits, vals) in zip(O.TABLE_IDS, specs)] == O.dht_of(data)
    assert len(specs) == (2 if CASES[name].cn == 1 else 4)
    for t, (bits, vals) in enumerate(specs):
        counted = np.nonzero(hist[t])[0].tolist()
        assert sum(bits) == len(counted) and len(bits) == 16                    # BITS counts the distinct symbols; none above 16
        assert sorted(vals) == counted                                         # HUFFVAL holds exactly the counted symbols
        assert sum(Fraction(n, 2 ** (i + 1)) for i, n in enumerate(bits)) < 1  # Kraft: the reserved code point stays free
        _, length = R.code_table((bits, vals))
        assert all(1 <= length[s] <= 16 for s in counted)
        assert not any(t % 2 == 0 and s > 11 for s in counted)                 # a DC table has the twelve categories at the most
    assert hist[:, 16:][[0, 2]].sum() == 0 and all(max(b for b, n in enumerate(s[0], 1) if n) <= 12 for s in specs[0::2])


def test_flat_block_gets_one_bit_codes():
    hist, specs, data, std, _ = K.reference(K.FLAT)
    assert hist.sum() == 2 and specs == [([1] + [0] * 15, [0]), ([1] + [0] * 15, [0])]
    assert len(K.scan_of(data)) == len(K.scan_of(std)) == 1 and len(data) < len(std)


def test_histograms_count_what_the_plain_coder_emits():
    for name in ("restart1_17x9", "noise_16x16_420", "bgra"):
        c = CASES[name]
        g = R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart)
        zz = R.coefficients(np.ascontiguousarray(c.image()), c.quality, c.subsampling)
        diff = R.dc_differences(zz, g)
        want = np.zeros((4, 256), np.int64)
        for b in range(g.nblocks):
            t = min(int(g.comp[b % g.bpm]), 1)
            want[2 * t, abs(int(diff[b])).bit_length()] += 1
            run = 0
            for k in range(1, 64):
                v = int(zz[b, k])
                if v == 0:
                    run += 1
                    continue
                want[2 * t + 1, 0xF0] += run >> 4
                want[2 * t + 1, (run & 15) << 4 | abs(v).bit_length()] += 1
                run = 0
            want[2 * t + 1, 0] += run > 0
        assert np.array_equal(K.reference(name)[0], want), name
    # every interval of restart1_17x9 starts at a prediction of 0: the differences of its first blocks are the DCs themselves
    c = CASES["restart1_17x9"]
    g = R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart)
    zz = R.coefficients(np.ascontiguousarray(c.image()), c.quality, c.subsampling)
    assert g.restart == 1 and g.nint > 1
    carried = R.dc_differences(zz, R.Geom(c.h, c.w, c.cn, c.subsampling, g.nmcu))
    assert not np.array_equal(np.bincount(R._size(carried), minlength=12), np.bincount(R._size(R.dc_differences(zz, g)), minlength=12))


def test_the_limit_to_16_bits_acts_on_the_docs_crop():
    for name in K.LIMITED:
        hist, specs, _, _, sizes = K.reference(name)
        longest = [max(s) for s in sizes]
        print(name, "longest code before the limit, by table:", longest)
        assert longest[1] > 16, (name, longest)                   # luminance AC
        for bits, vals in specs:
            _, length = R.code_table((bits, vals))
            assert length.max() <= 16
    assert max(K.reference("docs_444_q100")[4][3]) > 16           # chrominance AC too
    assert all(max(s) <= 16 for n in CASES if n not in K.LIMITED for s in K.reference(n)[4])


@pytest.mark.parametrize("name", list(CASES))
def test_optimised_file_is_smaller_and_within_the_bound(name):
    c = CASES[name]
    _, _, data, std, _ = K.reference(name)
    print(name, "file", len(std), "->", len(data), "scan", len(K.scan_of(std)), "->", len(K.scan_of(data)))
    assert len(K.scan_of(data)) <= R.bound(c.h, c.w, c.cn, c.subsampling, c.restart)
    if name == K.FLAT:
        assert len(K.scan_of(data)) == len(K.scan_of(std)) == 1 and len(data) < len(std)
    else:
        assert len(data) < len(std) and len(K.scan_of(data)) < len(K.scan_of(std))
    # a block of the optimised scan stays within the bytes the workspace gives every block (208): a DC token is 23 bits at the most
    g = R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart)
    zz = R.coefficients(np.ascontiguousarray(c.image()), c.quality, c.subsampling)
    with O._coder_tables(K.reference(name)[1]):
        assert R.block_bits(zz, g).max() <= 23 + 63 * 26 <= 8 * ((R.MAX_BLOCK_BITS + 7) // 8)


# ---- the product's arithmetic on the host -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_product_host_code_equals_restatement(opt_emul, name):
    hist, codes, data = _emul(opt_emul, CASES[name])
    whist, specs, wdata, _, _ = K.reference(name)
    assert np.array_equal(hist.astype(np.int64), whist)
    for t, spec in enumerate(specs):
        code, length = R.code_table(spec)
        n = 256 if t % 2 else 16
        got = codes[32 + (t // 2) * 256:][:256] if t % 2 else codes[(t // 2) * 16:][:16]
        assert np.array_equal(got.astype(np.int64), (length[:n] << 16) | code[:n]), (name, t)
    assert data == wdata


def test_builder_on_synthetic_counts(opt_emul):
    """the builder alone against the restatement: counts that double give the longest codes a table can have before the limit (one
    more bit per symbol), equal counts the tie rule, sums above 2^32 the 64-bit arithmetic"""
    rng = R._rng(300)
    tables = {"doubling_40": [1 << i for i in range(40)], "doubling_from_2^10": [1 << (10 + i) for i in range(30)],
              "equal_256": [7] * 256, "equal_162": [1] * 162, "one": [0, 0, 5], "two": [3, 0, 3],
              "random_sparse": (rng.integers(0, 50, 256) * (rng.random(256) < 0.4)).tolist(),
              "random_wide": (rng.integers(1, 1 << 32, 256)).tolist()}  # (a frequency stays below 2^40, as an image's does)
    assert max(O.code_sizes(tables["doubling_40"])) == 40 and max(O.code_sizes(tables["doubling_from_2^10"])) == 30
    lib = opt_emul
    lib.jpeg_opt_emul_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.jpeg_opt_emul_table.restype = C.c_uint32
    for name, counts in tables.items():
        counts = counts + [0] * (256 - len(counts))
        bits, vals = O.optimal_table(counts)
        assert sum(Fraction(n, 2 ** (i + 1)) for i, n in enumerate(bits)) < 1 and sorted(vals) == [i for i, c in enumerate(counts) if c]
        arr, codes, body = np.array(counts, np.uint64), np.zeros(256, np.uint32), np.zeros(16 + 256, np.uint8)
        n = lib.jpeg_opt_emul_table(arr.ctypes.data, 256, codes.ctypes.data, body.ctypes.data)
        assert body[:n].tolist() == bits + vals, name
        code, length = R.code_table((bits, vals))
        assert np.array_equal(codes.astype(np.int64), (length << 16) | code), name


# ---- the library without a device ---------------------------------------------------------------------------------------------------
def test_header_entry_and_argument_checks_without_device(product_lib):
    lib = product_lib
    lib.v1c_jpeg_header_opt.restype = C.c_int64
    lib.v1c_jpeg_header_opt.argtypes = [C.c_int] * 6 + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
    head = np.zeros(2048, np.uint8)
    for name in ("noise_16x16_420", K.FLAT, "bgra", "docs_444_q100"):
        c = CASES[name]
        g = R.Geom(c.h, c.w, c.cn, c.subsampling, c.restart)
        specs = K.reference(name)[1]
        body = np.frombuffer(O.dht_body(specs), np.uint8).copy()
        assert body.size <= DHT_MAX
        n = lib.v1c_jpeg_header_opt(c.h, c.w, c.cn, c.quality, R.SUBSAMPLINGS[c.subsampling], c.restart, body.ctypes.data, body.size,
                                    head.ctypes.data, head.size)
        assert head[:n].tobytes() == O.headers(g, c.quality, specs)
    c = CASES["noise_16x16_420"]
    body = np.frombuffer(O.dht_body(K.reference("noise_16x16_420")[1]), np.uint8).copy()
    call = lambda **k: lib.v1c_jpeg_header_opt(*[k.get(a, d) for a, d in [("h", 16), ("w", 16), ("cn", 3), ("q", 95), ("sub", 2), ("r", 1)]],  # noqa: E731
                                               k.get("dht", body.ctypes.data), k.get("n", body.size), k.get("out", head.ctypes.data), k.get("cap", 2048))
    assert call() > 0
    assert call(n=body.size - 1) == -1 and "dht" in lib.v1c_last_error().decode()      # not whole tables
    assert call(cn=1) == -1                                                             # four tables for one component
    assert call(dht=None) == -1 and call(out=None) == -1 and call(q=0) == -1 and call(cap=100) == -1

    lib.v1c_jpeg_encode_opt.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    buf, out, dht = np.zeros(1 << 16, np.uint8), np.zeros(1 << 20, np.uint8), np.zeros(DHT_MAX, np.uint8)
    size, dsize = C.c_uint64(0), C.c_uint32(0)

    def enc(img=buf.ctypes.data, h=64, w=64, pitch=192, cn=3, quality=95, sub=2, restart=4, dst=out.ctypes.data, cap=1 << 20, sz=C.byref(size),
            d=dht.ctypes.data, ds=C.byref(dsize)):
        return lib.v1c_jpeg_encode_opt(0, None, img, h, w, pitch, cn, quality, sub, restart, dst, cap, sz, d, ds)

    err = lambda: lib.v1c_last_error().decode()  # noqa: E731
    assert enc(cn=2) == -1 and "cn" in err() and enc(quality=0) == -1 and enc(sub=1) == -1 and enc(restart=0) == -1
    assert enc(img=None) == -1 and enc(d=None) == -1 and "NULL" in err() and enc(ds=None) == -1 and enc(sz=None) == -1
    assert enc(cap=1000) == -1 and "capacity" in err() and enc(pitch=191) == -1 and "pitch" in err()
    lib.v1c_jpeg_encode_batch_opt.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    assert lib.v1c_jpeg_encode_batch_opt(0, None, 0, None, 0, None) == 0 and lib.v1c_jpeg_encode_batch_opt(0, None, 1, None, 0, None) == -1
    from vr180_convert_amd import jpeg_device as J

    assert C.sizeof(J.JpegImageOpt) == C.sizeof(J.JpegImage) + 8 + DHT_MAX + 4 and J.DHT_MAX == DHT_MAX
    bad = (J.JpegImageOpt * 2)()
    bad[0] = J.JpegImageOpt(buf.ctypes.data, 8, 8, 24, 3, 95, 2, 1, out.ctypes.data, 1 << 20, 0, 1)
    bad[1] = J.JpegImageOpt(buf.ctypes.data, 8, 8, 24, 2, 95, 2, 1, out.ctypes.data, 1 << 20, 0, 1)
    assert lib.v1c_jpeg_encode_batch_opt(0, None, 2, bad, 0, None) == -1 and "image 1" in err()


def test_kernels_jpeg_opt_use_no_scratch_and_spill_nothing(tmp_path, product_lib):
    from test_resource_budget import kernel_metadata

    obj = ROOT / "vr180_convert_amd" / "csrc" / "kernels_jpeg_opt.o"
    assert obj.exists(), "kernels_jpeg_opt.o is built by __graft_entry__.build() / make"
    kernels = kernel_metadata(tmp_path, obj)
    names = [k[".name"] for k in kernels]
    assert len(names) == 2 and any("k_jpego_hist" in n for n in names) and any("k_jpego_build" in n for n in names), names
    bad = [(k[".name"], k[".private_segment_fixed_size"], k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for k in kernels
           if k[".private_segment_fixed_size"] or k[".sgpr_spill_count"] or k[".vgpr_spill_count"]]
    assert not bad, bad
    assert all(k[".wavefront_size"] == 64 for k in kernels)


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
def test_optimize_reaches_the_writers(tmp_path, monkeypatch):
    import inspect

    import torch

    from vr180_convert_amd import jpeg_device as J
    from vr180_convert_amd import remapper

    for f in (J.encode_jpeg_tensor, J.imwrite_jpeg_tensor, J.encode_jpeg_tensors, J.imwrite_jpeg_tensors):
        assert inspect.signature(f).parameters["optimize"].default is False
    for f in (remapper.apply, remapper.apply_lr):
        assert inspect.signature(f).parameters["device_jpeg_optimize"].default in (None, False)
    with pytest.raises(TypeError):
        J.encode_jpeg_tensor(torch.zeros((4, 4, 3), dtype=torch.uint8), optimize=True)
    with pytest.raises(ValueError):
        list(J._batch_parts([], 95, "420", None, None, optimize=[True]))


def test_cli_flag_reaches_apply_and_apply_lr(tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from vr180_convert_amd import _io, cli, remapper, synth

    seen = []
    monkeypatch.setattr(remapper, "apply_lr", lambda *a, **k: seen.append(("lr", k.get("device_jpeg"), k.get("device_jpeg_optimize"))))
    monkeypatch.setattr(remapper, "apply", lambda *a, **k: seen.append(("s", k.get("device_jpeg"), k.get("device_jpeg_optimize"))))
    img = tmp_path / "a.png"
    _io.imwrite(img, synth.pattern(64, 64))
    run = CliRunner().invoke
    base = ["--radius", "max", "--size", "32x32", "--out-path", str(tmp_path / "o.jpg")]
    assert run(cli.app, ["lr", str(img), str(img), *base, "--device-jpeg", "--device-jpeg-optimize"]).exit_code == 0
    assert run(cli.app, ["s", str(img), *base, "--device-jpeg-batch", "--device-jpeg-optimize"]).exit_code == 0
    assert run(cli.app, ["s", str(img), *base, "--device-jpeg"]).exit_code == 0
    assert seen == [("lr", True, True), ("s", "batch", True), ("s", True, None)]
