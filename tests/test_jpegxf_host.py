"""The lossless JPEG composer without a GPU: the restatement (jpgxf_ref.py) against mathematics -- a float64 inverse DCT of every
transformed block is the geometric transform of the source block's --, against a plain per-block loop, against Pillow's pixels and
against the transcoder's restatement (code 0, round trips, the join of a split); the product's host code (jpegxf_core.hpp,
jpegxf_host.hpp) against the restatement, byte for byte; what is refused, by the restatement, the harness, the library's host-only
entries and the Python layer, none of which touches a device; the EXIF orientations; the stand-alone sanitizer run; the resource notes
of kernels_jpegxf.o."""
import ctypes as C
import io
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jpg_cases as PC
import jpg_opt_ref as O
import jpg_ref as R
import jpgdec_cases as JC
import jpgdec_ref as D
import jpgdmg_cases as M
import jpgxc_cases as XK
import jpgxc_ref as X
import jpgxf_cases as K
import jpgxf_ref as F

ROOT = Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "host_jpegxf" / "jpegxf_emul.hip"
CASES = K.cases()
CODES = {F.Unsupported: -2, F.Invalid: -1}

# The most that Pillow's pixels of a transformed file differ from the transformed pixels of the source, over the all_codes_* files of
# this module, measured on the RESTATEMENT's outputs on the CPU: libjpeg's inverse DCT does not round
# symmetrically under a mirror of the columns or a transpose.  The tests assert that maximum plus one level.  flip_v is exact.
PILLOW_MAX = {"gray": 1, "444": 3}


def spec_words(outputs, src):
    """the outputs as the harness and the sanitizer program take them"""
    words = []
    for o in outputs:
        r = o.get("restart_mcus")
        if r is None:
            r = min(65535, -(-o["width"] // (src.mw if src is not None else 8)))
        words += [o["width"], o["height"], r, int(bool(o.get("optimize"))), len(o["regions"])]
        for reg in o["regions"]:
            words += [reg[0], F.code_of(reg[1]) if not isinstance(reg[1], int) else reg[1]] + list(reg[2:])
    return words


def _first_source(datas):
    try:
        return X.Source(datas[0])
    except Exception:  # noqa: BLE001 (a refused first file: its MCU width decides nothing)
        return None


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_jpegxf") / "libjpegxf_emul.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-fno-fast-math", "-o", str(out),
                    str(HARNESS)], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(out))
    lib.jxf_emul_compose.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
                                     C.c_void_p]
    lib.jxf_emul_tables.argtypes = [C.c_void_p, C.c_void_p]
    lib.jxf_emul_source_blocks.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    return lib


def run_emul(lib, datas, outputs, S=0):
    """(return code, [(header, file), ...], the damaged source) of the host build"""
    words = np.array(spec_words(outputs, _first_source(datas)), np.int32)
    blob = b"".join(datas)
    lens = np.array([len(d) for d in datas], np.uint64)
    files = np.zeros(1 << 21, np.uint8)
    sizes = np.zeros(2 * max(len(outputs), 1), np.uint64)
    damaged = C.c_int(-1)
    rc = lib.jxf_emul_compose(blob, lens.ctypes.data, len(datas), S, words.ctypes.data, len(words), len(outputs), files.ctypes.data, files.size,
                              sizes.ctypes.data, C.addressof(damaged))
    out, at = [], 0
    if rc == 0:
        for i in range(len(outputs)):
            head, total = int(sizes[2 * i]), int(sizes[2 * i + 1])
            out.append((files[at:at + head].tobytes(), files[at:at + total].tobytes()))
            at += total
    return rc, out, damaged.value


def _coefficients(data):
    """(info, (nblocks, 64) coefficients with the DC a value) of a file, by the decoder's restatement"""
    d = D.decode(data, check=False)
    return d.info, D.dc_values(d.info, d.coef)


def _pixels(a, code):
    """the geometric transform of an image: transpose first, then mirror x, then mirror y"""
    if code & 4:
        a = np.swapaxes(a, 0, 1)
    if code & 1:
        a = a[:, ::-1]
    if code & 2:
        a = a[::-1]
    return a


# ---- the formulas against mathematics ----------------------------------------------------------------------------------------------------
def _idct_basis():
    k = np.arange(8)
    c = np.where(k == 0, np.sqrt(0.125), 0.5)
    return c[:, None] * np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16)  # [frequency, sample]


def test_transformed_blocks_are_the_transformed_samples_in_float64():
    """every code's transformed block, dequantised with the table the header writes (the source's, transposed where the code
    transposes), through a float64 inverse DCT is the geometric transform of the source block's float64 inverse DCT, to 1e-9 of full
    scale: the formulas are held to mathematics, not to a codec"""
    rng = np.random.default_rng(20)
    B = _idct_basis()
    q = rng.integers(1, 256, 64)                         # an asymmetric table, row-major
    blocks = rng.integers(-1023, 1024, (50, 64))         # zigzag order
    blocks[:, 0] = rng.integers(-1024, 1024, 50)

    def samples(zz, table):
        nat = np.zeros((len(zz), 64))
        nat[:, R.ZIGZAG] = zz
        f = (nat * table).reshape(-1, 8, 8)              # F[v][u]
        return np.einsum("vy,nvu,ux->nyx", B, f, B)

    want0 = samples(blocks, q)
    for code in range(8):
        moved = np.stack([F.transform_mcus(b.reshape(1, 1, 1, 64), code, 1, 1).reshape(64) for b in blocks])  # (one MCU each)
        table = q.reshape(8, 8).T.reshape(64) if code & 4 else q
        got = samples(moved, table)
        want = np.stack([_pixels(b, code) for b in want0])
        assert np.abs(got - want).max() <= 1e-9 * 256 * 8, code  # (full scale: 8-bit samples; the sums of 64 terms keep well inside)
        assert np.array_equal(moved[:, 0], blocks[:, 0])  # the DC never changes
    assert not np.array_equal(F.TZ, np.arange(64)) and np.array_equal(F.TZ[F.TZ], np.arange(64))


def _loop_gather(srcs, out, g):
    """the output's coefficients by a plain loop over blocks and coefficients: the issue's rules, one at a time"""
    a = srcs[0].info
    hs, vs, bpm = a.hs, a.vs, a.bpm
    got = np.zeros((g.nblocks, 64), np.int64)
    for si, tr, sx, sy, nx, ny, dx, dy in out["regions"]:
        code = F.code_of(tr)
        s = srcs[si].info
        NX, NY = (ny, nx) if code & 4 else (nx, ny)
        for J in range(NY):
            for I in range(NX):
                for k in range(bpm):
                    i, j = I, J
                    bx, by = k % hs, k // hs
                    if code & 1:
                        i, bx = NX - 1 - i, hs - 1 - bx
                    if code & 2:
                        j, by = NY - 1 - j, vs - 1 - by
                    if code & 4:
                        i, j, bx, by = j, i, by, bx
                    sk = by * hs + bx if k < hs * vs else k
                    blk = srcs[si].coef[((sy + j) * s.mcux + sx + i) * bpm + sk]
                    dst = got[((dy + J) * g.mcux + dx + I) * bpm + k]
                    for z in range(64):
                        v, u = divmod(int(R.ZIGZAG[z]), 8)
                        sz = int(np.nonzero(R.ZIGZAG == (u * 8 + v if code & 4 else v * 8 + u))[0][0])
                        sign = (-1 if code & 1 and u & 1 else 1) * (-1 if code & 2 and v & 1 else 1)
                        dst[z] = sign * int(blk[sz])
    return got


LOOPED = [n for n in CASES if n.startswith(("all_codes_3x2", "mosaic", "join_right", "partial_trimmed", "transposed_rectangle", "mixed_transpose",
                                            "coefficient_limits", "dqt16"))]


@pytest.mark.parametrize("name", LOOPED)
def test_outputs_hold_the_coefficients_of_a_plain_loop(name):
    """jpgdec_ref's decode of every output gives the coefficients of a per-block, per-coefficient Python loop over the sources', the
    quantisation tables of region 0's source -- transposed where region 0 transposes --, the sampling factors and the size asked for"""
    datas, outputs = CASES[name]
    srcs = F.sources_of(list(datas))
    for out, made in zip(outputs, K.reference(name)):
        t, got = _coefficients(made)
        g = F.check(srcs, out)
        s = srcs[out["regions"][0][0]].info
        assert (t.h, t.w, t.nc, t.hs, t.vs) == (out["height"], out["width"], s.nc, s.hs, s.vs)
        tr = bool(F.code_of(out["regions"][0][1]) & 4)
        for c in range(s.nc):
            want = np.asarray(s.q[s.tq[c]])
            assert np.array_equal(t.q[t.tq[c]], want.reshape(8, 8).T.reshape(64) if tr else want), name
        assert np.array_equal(got.astype(np.int64), _loop_gather(srcs, out, g)), name


def test_case_list_sits_on_the_boundaries_it_is_for():
    blocks = {F.check(F.sources_of(list(d)), o).nblocks for n, (d, outs) in CASES.items() if n.startswith("blocks_") for o in outs}
    assert {31, 32, 33, 255, 256, 257, 258} <= blocks
    for kind in K.KINDS:
        want = {0, 1, 2, 3} if kind == "422" else set(range(8))
        for size in ("1x1", "1x2", "2x1", "3x2"):
            assert {o["regions"][0][1] for o in CASES[f"all_codes_{size}_{kind}"][1]} == want
        assert [D.parse(CASES[f"source_dri{r}_{kind}"][0][0]).restart for r in (1, 2, 7)] == [1, 2, 7]
        assert len(CASES[f"mosaic_{kind}"][0]) == 4 and len({r[1] for r in CASES[f"mosaic_{kind}"][1][0]["regions"]}) == 4
        s = D.parse(CASES[f"partial_trimmed_{kind}"][0][0])
        m, n = K.KINDS[kind][2:]
        assert s.w % m and s.h % n
        assert {bool(o.get("optimize")) for o in CASES[f"optimize_mixed_{kind}"][1]} == {True, False}
    assert {o.get("restart_mcus") for _, outs in CASES.values() for o in outs} >= {None, 0, 1}
    s, coef = _coefficients(CASES["coefficient_limits"][0][0])
    assert coef[:, 0].min() == -1024 and coef[:, 0].max() == 1023 and coef[:, 1:].min() == -1023 and coef[:, 1:].max() == 1023
    for made in K.reference("coefficient_limits"):
        t, got = _coefficients(made)
        assert np.abs(got[:, 1:]).max() == 1023
    wide = D.parse(CASES["dqt16_transposed"][0][0])
    assert wide.q[wide.tq[0]].max() == 300 and not np.array_equal(wide.q[wide.tq[0]], wide.q[wide.tq[0]].reshape(8, 8).T.reshape(64))
    assert b"\xff\xc1" in K.reference("dqt16_transposed")[0][:400]
    assert np.array_equal(D.parse(K.reference("dqt16_transposed")[0]).q[0], wide.q[wide.tq[0]].reshape(8, 8).T.reshape(64))


# ---- the restatement against Pillow ------------------------------------------------------------------------------------------------------
def _pillow_differences(kind):
    """{code: the largest difference between Pillow's pixels of the restatement's output and the transformed pixels of the source} over
    the kind's all_codes_* files"""
    worst = {}
    for size in ("1x1", "1x2", "2x1", "3x2"):
        datas, outputs = CASES[f"all_codes_{size}_{kind}"]
        src = R.decode(datas[0]).astype(np.int64)
        for out, made in zip(outputs, K.reference(f"all_codes_{size}_{kind}")):
            code = out["regions"][0][1]
            got = R.decode(made).astype(np.int64)
            want = _pixels(src, code)
            assert got.shape == want.shape
            worst[code] = max(worst.get(code, 0), int(np.abs(got - want).max()))
    return worst


@pytest.mark.parametrize("kind", ["gray", "444"])
def test_pillow_s_pixels_of_transformed_files(kind):
    """flip_v exactly (libjpeg's column pass swaps rows exactly when the odd rows change sign); every other code within the measured
    maximum of the restatement's outputs plus one level"""
    worst = _pillow_differences(kind)
    print(kind, worst)
    assert worst[0] == 0 and worst[2] == 0
    assert all(v <= PILLOW_MAX[kind] + 1 for v in worst.values()), worst


# ---- the restatement against the transcoder's ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(K.KINDS))
def test_a_code_and_its_inverse_give_the_transcoded_file_back(kind):
    data = CASES[f"all_codes_3x2_{kind}"][0][0]
    plain = X.transcode_jpeg(data)
    for code in K.codes_of(kind):
        once = F.transform_jpeg(data, F.NAMES[code])
        assert F.transform_jpeg(once, F.NAMES[F.INVERSE[code]]) == plain, code
        assert code == 0 or once != plain


def test_join_of_a_split_is_the_whole_image_transcode():
    for name in ("swap_2x2_gray", "swap_2x2_444", "swap_2x2_422", "swap_2x2_420", "swap_dri7_420", "noise_q100_444_swap"):
        data = XK.cases()[name][0]
        left, right = X.split_sbs_jpeg(data)
        assert F.join_sbs_jpeg(left, right) == X.transcode_jpeg(data), name
        assert F.join_sbs_jpeg(left, right, optimize=True, restart_mcus=0) == X.transcode_jpeg(data, optimize=True, restart_mcus=0), name


def _as_compose(outputs):
    return [dict(o, regions=[(0, 0) + tuple(r) for r in o["regions"]]) for o in outputs]


@pytest.mark.parametrize("name", list(XK.cases()))
def test_code_0_is_the_transcoder(emul, name):
    """code 0 through the composer -- restatement and host build -- is jpgxc_ref.transcode byte for byte on every case of the transcoder"""
    data, outputs = XK.cases()[name]
    want = list(XK.reference(name))
    assert F.compose([data], _as_compose(outputs)) == want
    rc, made, _ = run_emul(emul, [data], _as_compose(outputs))
    assert rc == 0 and [m[1] for m in made] == want


# ---- the product's host code against the restatement -------------------------------------------------------------------------------------
def test_tables_of_the_host_build(emul):
    """jpegxf_core.hpp's zigzag transpose and sign masks, built at compile time, against the restatement's, built from jpg_ref's table"""
    frm, masks = np.zeros(8 * 64, np.uint8), np.zeros(8, np.uint64)
    assert emul.jxf_emul_tables(frm.ctypes.data, masks.ctypes.data) == 1
    for code in range(8):
        assert np.array_equal(frm[64 * code:64 * code + 64], F.TZ if code & 4 else np.arange(64)), code
        sign = (F.SIGN_X if code & 1 else 1) * (F.SIGN_Y if code & 2 else 1) * np.ones(64, np.int64)
        assert int(masks[code]) == sum(1 << z for z in range(64) if sign[z] < 0), code
        assert not int(masks[code]) & 1


@pytest.mark.parametrize("name", list(CASES))
def test_host_build_equals_restatement(emul, name):
    """header and file, byte for byte, at two subsequence sizes"""
    datas, outputs = CASES[name]
    srcs = F.sources_of(list(datas))
    for S in (256, 0):
        rc, made, _ = run_emul(emul, datas, outputs, S)
        assert rc == 0, (name, rc)
        for (head, whole), out, want in zip(made, outputs, K.reference(name)):
            _, want_head, want_scan = F.parts(srcs, out)
            assert head == want_head, name
            assert whole == want == want_head + want_scan + b"\xff\xd9", name


def test_source_blocks_of_the_host_build(emul):
    """jpegxf_core.hpp's block map against the restatement's transform of MCU and block indices, uncovered MCUs included"""
    rng = np.random.default_rng(4)
    for hs, vs, bpm in ((1, 1, 1), (1, 1, 3), (2, 1, 4), (2, 2, 6)):
        for _ in range(40):
            code = int(rng.integers(0, 8)) & (3 if hs != vs else 7)
            smx, smy = int(rng.integers(1, 7)), int(rng.integers(1, 6))
            nx, ny = int(rng.integers(1, smx + 1)), int(rng.integers(1, smy + 1))
            sx, sy = int(rng.integers(0, smx - nx + 1)), int(rng.integers(0, smy - ny + 1))
            NX, NY = F.placed(code, nx, ny)
            dx, dy = int(rng.integers(0, 3)), int(rng.integers(0, 3))
            dmx, dmy = dx + NX + int(rng.integers(0, 2)), dy + NY + int(rng.integers(0, 2))
            index = np.zeros((smy, smx, bpm, 64), np.int64)
            index[..., 0] = np.arange(smx * smy * bpm).reshape(smy, smx, bpm)
            want = np.full((dmy, dmx, bpm), 0xFFFFFFFF, np.int64)
            want[dy:dy + NY, dx:dx + NX] = F.transform_mcus(index[sy:sy + ny, sx:sx + nx], code, hs, vs)[..., 0]
            got = np.zeros(3 * dmx * dmy * bpm, np.uint32)
            reg = np.array([2, code, sx, sy, nx, ny, dx, dy, smx], np.uint32)
            emul.jxf_emul_source_blocks(reg.ctypes.data, 1, dmx, dmy, hs, vs, bpm, got.ctypes.data)
            got = got.reshape(-1, 3).astype(np.int64)
            assert np.array_equal(got[:, 2], want.reshape(-1)), (hs, vs, code)
            held = got[:, 2] != 0xFFFFFFFF
            assert np.all(got[held, 0] == 2) and np.all(got[held, 1] == code)


# ---- what is refused -------------------------------------------------------------------------------------------------------------------
def test_refusals_by_the_restatement_and_the_host_build(emul):
    for name, (datas, outputs, exc) in K.refused().items():
        with pytest.raises(exc):
            F.compose(list(datas), outputs)
        rc, _, _ = run_emul(emul, datas, outputs)
        assert rc == CODES[exc], (name, rc)
    for name, (datas, outputs, by_parse) in K.corrupt().items():
        if by_parse:
            with pytest.raises(D.Corrupt):
                F.compose(list(datas), outputs)
        rc, _, damaged = run_emul(emul, datas, outputs)
        assert rc == -5 and (by_parse or damaged == 1), (name, rc, damaged)
    for name, (datas, outputs) in K.out_of_range().items():
        with pytest.raises(F.Unsupported):
            F.compose(list(datas), outputs)
        rc, _, _ = run_emul(emul, datas, outputs)
        assert rc == -2, (name, rc)


def _xf_call(datas, outputs):
    from vr180_convert_amd.jpeg_compose_device import XfOutput, XfRegion, XfSource

    srcs = (XfSource * max(len(datas), 1))(*[XfSource(d, len(d)) for d in datas])
    outs = (XfOutput * len(outputs))()
    keep = [srcs]
    src = _first_source(datas)
    for o, spec in zip(outs, outputs):
        regs = [(r[0], F.code_of(r[1]) if not isinstance(r[1], int) else r[1]) + tuple(r[2:]) for r in spec["regions"]]
        arr = (XfRegion * max(len(regs), 1))(*[XfRegion(*r) for r in regs])
        keep.append(arr)
        r = spec.get("restart_mcus")
        o.width, o.height = spec["width"], spec["height"]
        o.restart_mcus = min(65535, -(-spec["width"] // (src.mw if src else 8))) if r is None else r
        o.optimize, o.nregions, o.regions = int(bool(spec.get("optimize"))), len(regs), arr
    return srcs, outs, keep


def test_library_refuses_without_a_device(product_lib):
    """the host-only entries of the C ABI, and v1c_jpeg_compose itself, whose checks all come before its first device call (device -1
    would be its next complaint)"""
    from vr180_convert_amd import _native

    lib = _native.lib()
    buf = np.zeros(1 << 20, np.uint8)
    for name, (datas, outputs, exc) in K.refused().items():
        srcs, outs, keep = _xf_call(datas, outputs)
        assert lib.v1c_jpeg_compose_check(len(datas), srcs, len(outputs), outs, None) == CODES[exc], name
        for o in outs:
            o.out_host, o.capacity = buf.ctypes.data, buf.size
        assert lib.v1c_jpeg_compose(-1, None, len(datas), srcs, len(outputs), outs, 0, None) == CODES[exc], name
    for name, (datas, outputs, by_parse) in K.corrupt().items():
        srcs, outs, keep = _xf_call(datas, outputs)
        pos = (C.c_uint64 * 2)()
        assert lib.v1c_jpeg_compose_check(2, srcs, len(outputs), outs, pos) == (-5 if by_parse else 0), name
        assert pos[0] == 0
    for name, (datas, outputs) in CASES.items():
        srcs, outs, keep = _xf_call(datas, outputs)
        assert lib.v1c_jpeg_compose_check(len(datas), srcs, len(outputs), outs, None) == 0, name
        # with every check passed the next complaint is the device's: nothing before it touched one
        for o in outs:
            o.out_host, o.capacity = buf.ctypes.data, 1 << 40
        assert lib.v1c_jpeg_compose(-1, None, len(datas), srcs, len(outputs), outs, 0, None) == -4, name
        for o in outs:
            o.capacity = 16
        assert lib.v1c_jpeg_compose(-1, None, len(datas), srcs, len(outputs), outs, 0, None) == -1 and b"capacity" in lib.v1c_last_error()
    datas, outputs = CASES["join_420"]
    srcs, outs, keep = _xf_call(datas, outputs)
    assert lib.v1c_jpeg_compose_check(0, srcs, 1, outs, None) == -1 and lib.v1c_jpeg_compose_check(2, None, 1, outs, None) == -1
    assert lib.v1c_jpeg_compose_check(2, srcs, 0, outs, None) == -1 and lib.v1c_jpeg_compose_check(2, srcs, 17, outs, None) == -1
    assert lib.v1c_jpeg_compose_check(2, srcs, 1, None, None) == -1
    assert lib.v1c_jpeg_compose(0, None, 2, srcs, 1, outs, 100, None) == -1 and b"subseq_bits" in lib.v1c_last_error()


def test_library_header_and_bound_equal_the_restatement(product_lib):
    from vr180_convert_amd import _native

    lib = _native.lib()
    for name, (datas, outputs) in CASES.items():
        srcs = F.sources_of(list(datas))
        for out in outputs:
            g = F.check(srcs, out)
            zz, want_head, want_scan = F.parts(srcs, out)
            dht = O.dht_body(O.tables(zz, g)) if out.get("optimize") else None
            si, tr = out["regions"][0][:2]
            d = datas[si]
            head = (C.c_uint8 * 2048)()
            n = lib.v1c_jpeg_header_xf(d, len(d), out["width"], out["height"], g.dri, F.code_of(tr) >> 2, dht, len(dht) if dht else 0, head, 2048)
            assert n > 0 and bytes(head[:n]) == want_head, name
            bound = lib.v1c_jpeg_compose_bound(d, len(d), out["width"], out["height"], g.dri)
            assert bound == lib.v1c_jpeg_transcode_bound(d, len(d), out["width"], out["height"], g.dri) >= len(want_scan) > 0
    d = CASES["join_422"][0][0]
    head = (C.c_uint8 * 2048)()
    assert lib.v1c_jpeg_header_xf(d, len(d), 32, 32, 2, 1, None, 0, head, 2048) == -2 and b"4:4:0" in lib.v1c_last_error()
    assert lib.v1c_jpeg_header_xf(d, len(d), 32, 32, 2, 0, b"\x00" * 20, 20, head, 2048) == -1 and b"dht" in lib.v1c_last_error()
    assert lib.v1c_jpeg_header_xf(d, len(d), 32, 32, 2, 0, None, 0, head, 100) == -1 and lib.v1c_jpeg_header_xf(d, len(d), 0, 32, 2, 0, None, 0, head, 2048) == -1
    assert lib.v1c_jpeg_compose_bound(b"\xff\xd8\xff", 3, 32, 32, 2) == 0


def test_python_layer_refuses_before_any_device_call(monkeypatch):
    """NotImplementedError for files and region sets outside scope, CorruptJPEG for a damaged file, ValueError for geometry; the device
    is never asked for"""
    import vr180_convert_amd as V
    from vr180_convert_amd import jpeg_compose_device as T, remapper
    from vr180_convert_amd.jpeg_decode_device import CorruptJPEG

    def no_device(*a, **k):
        raise AssertionError("a refused call asked for the device")

    monkeypatch.setattr(remapper, "_device", no_device)
    assert V.compose_regions is T.compose_regions and V.transform_jpeg is T.transform_jpeg and V.join_sbs_jpeg is T.join_sbs_jpeg
    assert V.sbs_from_vr180_photo is T.sbs_from_vr180_photo and V.normalize_orientation_jpeg is T.normalize_orientation_jpeg

    def named(outputs):
        return [dict(o, regions=[(r[0], F.NAMES.get(r[1], r[1])) + tuple(r[2:]) for r in o["regions"]]) for o in outputs]

    for name, (datas, outputs, exc) in K.refused().items():
        want = NotImplementedError if exc is F.Unsupported else ValueError
        with pytest.raises(want):
            T.compose_regions(datas, named(outputs))
    for name, (datas, outputs, by_parse) in K.corrupt().items():
        if by_parse:
            with pytest.raises(CorruptJPEG):
                T.compose_regions(datas, named(outputs))
    part = CASES["partial_trimmed_420"][0][0]                       # 45 x 27 pixels of 16 x 16 MCUs
    for op in ("flip_h", "flip_v", "rot180", "rot90", "rot270", "transverse"):
        with pytest.raises(ValueError, match="MCU"):
            T.transform_jpeg(part, op)
    with pytest.raises(ValueError, match="transform"):
        T.transform_jpeg(part, "rot45")
    with pytest.raises(NotImplementedError):
        T.transform_jpeg(CASES["join_422"][0][0], "rot90")
    whole = CASES["join_420"][0][0]                                 # 48 x 32
    with pytest.raises(ValueError, match="left eye's width"):
        T.join_sbs_jpeg(part, part)
    with pytest.raises(ValueError, match="height"):
        T.join_sbs_jpeg(whole, whole, right_transform="rot90")
    with pytest.raises(ValueError):
        T.sbs_from_vr180_photo(whole)                               # no VR180 photo
    # the same geometry as the restatement's
    h, w, mw, mh = T.probe_mcu(part)
    src = X.Source(part)
    for code in range(8):
        assert T._transformed(h, w, mw, mh, code, True) == F.transformed_size(src, code, True)


# ---- EXIF orientation ------------------------------------------------------------------------------------------------------------------
def _with_exif(data, orientation, order):
    """the file with an APP1 Exif segment of one IFD entry, tag 0x0112, behind SOI"""
    e = "<" if order == "II" else ">"
    tiff = order.encode() + struct.pack(e + "HI", 42, 8) + struct.pack(e + "HHHIHH", 1, 0x0112, 3, 1, orientation, 0) + struct.pack(e + "I", 0)
    body = b"Exif\x00\x00" + tiff
    return data[:2] + b"\xff\xe1" + struct.pack(">H", len(body) + 2) + body + data[2:]


def test_exif_orientation_is_read_in_both_byte_orders_and_applied():
    """files of all eight orientations: the parser against Pillow's, the transform the table names against ImageOps.exif_transpose on
    the restatement's output, within the measured bound of the Pillow test"""
    from PIL import Image, ImageOps

    from vr180_convert_amd import jpeg_compose_device as T

    data = CASES["all_codes_3x2_444"][0][0]
    assert T.exif_orientation(data) == 1 and T.exif_orientation(b"\xff\xd8\xff\xd9") == 1
    for order in ("II", "MM"):
        for orientation in range(1, 9):
            tagged = _with_exif(data, orientation, order)
            im = Image.open(io.BytesIO(tagged))
            assert im.getexif().get(0x0112) == orientation == T.exif_orientation(tagged), (order, orientation)
            want = np.asarray(ImageOps.exif_transpose(im).convert("RGB")).astype(np.int64)
            made = F.transform_jpeg(tagged, T.EXIF_TRANSFORMS[orientation])
            got = np.asarray(Image.open(io.BytesIO(made)).convert("RGB")).astype(np.int64)
            assert Image.open(io.BytesIO(made)).getexif().get(0x0112) is None
            assert got.shape == want.shape and np.abs(got - want).max() <= PILLOW_MAX["444"] + 1, (order, orientation)
    assert T.exif_orientation(_with_exif(data, 9, "II")) == 1 and T.exif_orientation(_with_exif(data, 0, "MM")) == 1


# ---- the stand-alone sanitizer run -----------------------------------------------------------------------------------------------------
def test_standalone_sanitizer_run(tmp_path):
    """the host build as a program of its own under the address and undefined-behaviour sanitizers: every case, the refused and the
    corrupt ones, a second source truncated at every length and every damaged scan of tests/jpgdmg_cases.py as the second source of a
    join, from heap copies of exact sizes; any report fails the run"""
    exe = tmp_path / "jpegxf_san"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fno-fast-math", "-DJXF_MAIN", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(HARNESS)], check=True,
                   capture_output=True, timeout=600)
    lines, k = [], 0

    def add(datas, outputs, want):
        nonlocal k
        paths = []
        for d in datas:
            p = tmp_path / f"case_{k}.jpg"
            k += 1
            p.write_bytes(d)
            paths.append(p)
        lines.append(" ".join(str(v) for v in [want, len(datas)] + paths + [len(outputs)] + spec_words(outputs, _first_source(datas))))

    for name, (datas, outputs) in CASES.items():
        add(datas, outputs, 0)
    for name, (datas, outputs, exc) in K.refused().items():
        add(datas, outputs, CODES[exc])
    for name, (datas, outputs, by_parse) in K.corrupt().items():
        add(datas, outputs, -5)
    datas, outputs = CASES["join_right_rot180_420"]
    for n in list(range(0, 700, 7)) + list(range(700, len(datas[1]), 41)):
        add([datas[0], datas[1][:n]], outputs, -5)
    # the damaged scans of tests/jpgdmg_cases.py, which do reach the entropy decoder, as the second source of a join
    for x in M.sequential_cases():
        j = M.join_want(x.name)
        if j is not None:
            add([M.base_of(x), x.data], [j[0]], j[1])
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(manifest)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-3000:])
    assert len(r.stdout.strip().splitlines()) == 2 * len(lines)


# ---- the code object ---------------------------------------------------------------------------------------------------------------------
def test_kernels_jpegxf_use_no_scratch_and_spill_nothing(tmp_path, product_lib):
    from test_resource_budget import kernel_metadata

    obj = ROOT / "vr180_convert_amd" / "csrc" / "kernels_jpegxf.o"
    assert obj.exists(), "kernels_jpegxf.o is built by __graft_entry__.build() / make"
    kernels = kernel_metadata(tmp_path, obj)
    assert len(kernels) == 1 and "k_jxf_gather" in kernels[0][".name"]
    k = kernels[0]
    assert (k[".private_segment_fixed_size"], k[".sgpr_spill_count"], k[".vgpr_spill_count"]) == (0, 0, 0)
    assert k[".wavefront_size"] == 64 and k[".group_segment_fixed_size"] == 4096  # the transposing blocks' 128 bytes each
