"""16-bit and float32 images without a GPU: the float weight table, the product's wide sampler run on the host against the NumPy
restatement of the contract (wide_ref.py), the C ABI's argument checks, the Python type checks, the 16-bit PNG writer and the resource
budget of kernels_wide.o."""
import ctypes as C
import struct
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

import wide_ref as R

ROOT = Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "host_wide" / "wide_emul.hip"
DEPTH = {np.uint16: 2, np.float32: 5}
BORDER_VALUES = [70000, -3, 2.5, 1.5, 0.25, (70000, -3, 2.5, 1.5), (1.5, 0.25, -3)]


@pytest.fixture(scope="module")
def wide_emul(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_wide") / "libwide_emul.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-fno-fast-math", "-o", str(out),
                    str(HARNESS)], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(out))
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    lib.wide_remap_host.argtypes = [vp, i32, i32, i64, i32, i32, vp, i32, i32, i64, vp, vp, i32, i32, vp, vp]
    lib.wide_border_host.argtypes = [i32, vp, vp]
    return lib


def product_cval(lib, depth, value):
    """The product's saturation of a border value given as Python / cv2 does (a bare number: component 0 only)."""
    vals = [value] if np.isscalar(value) else list(value)
    bv = np.zeros(4, np.float64)
    bv[:len(vals)] = vals
    out = np.zeros(4, np.float32)
    lib.wide_border_host(depth, bv.ctypes.data, out.ctypes.data)
    return out


def product_ftab(lib, interp):
    k = R.taps_per_axis(interp)
    out = np.zeros((1024, k, k), np.float32)
    assert lib.v1c_build_ftab(interp, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("interp", [R.INTER_LINEAR, R.INTER_CUBIC, R.INTER_LANCZOS4])
def test_ftab_equals_restatement(product_lib, interp):
    got = product_ftab(product_lib, interp)
    want = R.ftab(interp)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("interp", [R.INTER_CUBIC, R.INTER_LANCZOS4])
def test_ftab_rounds_to_the_int16_table(product_lib, oracle_mod, interp):
    """saturate_cast<short>(rint(wf * 32768)) is the pinned int16 table at every tap outside the central 2 x 2, where only the
    saturation and the sum fix-up of initInterTab2D may move a value (its 2 x 2 is taps K/2 .. K/2 + 1 of each axis)."""
    wf = product_ftab(product_lib, interp)
    it = oracle_mod.build_itab(interp).astype(np.int64)
    k = wf.shape[1]
    r = np.clip(np.rint(wf.astype(np.float32) * np.float32(32768)), -32768, 32767).astype(np.int64)
    centre = np.zeros((k, k), bool)
    centre[k // 2:k // 2 + 2, k // 2:k // 2 + 2] = True
    assert np.array_equal(r[:, ~centre], it[:, ~centre])
    # inside it, the sum fix-up moves one tap by the rounding surplus at most (and 32768 saturates to 32767)
    assert np.abs(r[:, centre] - it[:, centre]).max() <= k * k


def random_maps(rng, h, w, src_h, src_w):
    """Coordinates inside, on and just outside every edge, far outside (+-1e6) and NaN."""
    xm = rng.uniform(-3.5, src_w + 2.5, (h, w)).astype(np.float32)
    ym = rng.uniform(-3.5, src_h + 2.5, (h, w)).astype(np.float32)
    edges_x = np.array([0, -0.5, -1, -1.02, src_w - 1, src_w - 0.5, src_w, src_w - 1.5, 0.49, -0.51, src_w - 0.49], np.float32)
    edges_y = np.array([0, -0.5, -1, -1.02, src_h - 1, src_h - 0.5, src_h, src_h - 1.5, 0.49, -0.51, src_h - 0.49], np.float32)
    sel = rng.random((h, w))
    xm = np.where(sel < 0.25, rng.choice(edges_x, (h, w)), xm)
    ym = np.where((sel > 0.15) & (sel < 0.4), rng.choice(edges_y, (h, w)), ym)
    # exact 1/32 buckets near the edges too
    xm = np.where((sel > 0.4) & (sel < 0.5), np.round(xm * 32) / 32, xm).astype(np.float32)
    special = rng.random((h, w))
    xm[special < 0.02] = 1e6
    ym[(special > 0.02) & (special < 0.04)] = -1e6
    xm[(special > 0.04) & (special < 0.06)] = np.nan
    ym[(special > 0.06) & (special < 0.07)] = np.nan
    return xm, ym


def random_source(rng, dtype, h, w, cn):
    if dtype == np.uint16:
        a = rng.integers(0, 65536, (h, w, cn)).astype(np.uint16)
        a[rng.random((h, w)) < 0.1] = 65535
        return a
    a = rng.normal(0.5, 2.0, (h, w, cn)).astype(np.float32)
    m = rng.random((h, w, cn))
    a[m < 0.01] = np.inf
    a[(m > 0.01) & (m < 0.02)] = -np.inf
    a[(m > 0.02) & (m < 0.03)] = np.nan
    return a


def host_remap(lib, ftab, src, xm, ym, interp, border, cval, dst):
    h, w, cn = src.shape
    dh, dw = xm.shape
    rc = lib.wide_remap_host(src.ctypes.data, h, w, src.strides[0], cn, DEPTH[src.dtype.type], dst.ctypes.data, dh, dw, dst.strides[0],
                             xm.ctypes.data, ym.ctypes.data, interp, border, cval.ctypes.data,
                             None if ftab is None else ftab.ctypes.data)
    assert rc == 0
    return dst


def same(got, want):
    if got.dtype == np.uint16:
        return got.tobytes() == want.tobytes()
    return np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("interp", [0, 1, 2, 3, 4])
def test_host_sampler_equals_restatement(product_lib, wide_emul, dtype, interp):
    rng = np.random.default_rng(1000 + 10 * interp + (dtype == np.float32))
    ftab = product_ftab(product_lib, interp) if interp in (R.INTER_CUBIC, R.INTER_LANCZOS4) else None
    case = 0
    for border in range(6):
        for cn in (1, 3, 4):
            for src_h, src_w in ((9, 13), (1, 7), (12, 2)):
                src = random_source(rng, dtype, src_h, src_w, cn)
                xm, ym = random_maps(rng, 17, 23, src_h, src_w)
                bv = BORDER_VALUES[case % len(BORDER_VALUES)]
                case += 1
                cval = product_cval(wide_emul, DEPTH[dtype], bv)  # (the product's saturation; the restatement saturates on its own)
                init = random_source(rng, dtype, 17, 23, cn)  # TRANSPARENT keeps these
                got = host_remap(wide_emul, ftab, src, xm, ym, interp, border, cval, init.copy())
                want = R.remap(src, xm, ym, interp, border, bv, dst=init)
                assert same(got, want), (dtype, interp, border, cn, (src_h, src_w), bv,
                                         int((~((got == want) | (np.isnan(got.astype(np.float32)) & np.isnan(want.astype(np.float32))))).sum()))


def test_border_saturation(wide_emul):
    """The product's saturate_cast of the border Scalar (v1c_core.hpp: border_component, what v1c_plan_create_ex uses)."""
    assert list(product_cval(wide_emul, 2, 70000)) == [65535, 0, 0, 0]
    assert list(product_cval(wide_emul, 2, (-3, 2.5, 1.5, 0.25))) == [0, 2, 2, 0]  # half to even
    assert list(product_cval(wide_emul, 2, (65535.5, 3.5, float("nan"), 1e300))) == [65535, 4, 0, 0]  # NaN, beyond int: 0
    assert list(product_cval(wide_emul, 5, (-3, 2.5, 1.5, 0.25))) == [-3, 2.5, 1.5, 0.25]
    assert list(product_cval(wide_emul, 5, (1e300, 0.1))) == [np.inf, np.float32(0.1), 0, 0]
    assert list(product_cval(wide_emul, 0, (300, 2.5, 3.5, -1))) == [255, 2, 4, 0]  # 8-bit: what v1c_plan_create has always done
    for bv in BORDER_VALUES:
        for dtype in (np.uint16, np.float32):
            assert np.array_equal(product_cval(wide_emul, DEPTH[dtype], bv), R.border_cval(bv, dtype))


def test_abi_checks_without_device(product_lib):
    from vr180_convert_amd import _abi

    h = C.c_void_p()
    ch = _abi.chain([_abi.op(_abi.OP_NORMALIZE, 0, [4, 4, 8]), _abi.op(_abi.OP_DENORMALIZE, 0, [4, 4, 4, 4])])
    bv = (C.c_double * 4)(0, 0, 0, 0)
    for depth in (1, 3, 4, 6, -1):
        assert product_lib.v1c_plan_create_ex(C.byref(h), 0, C.byref(ch), 8, 8, 8, 8, 3, depth, 1, 0, bv) == _abi.E_INVALID
        assert product_lib.v1c_remap_lut_ex(0, None, None, 8, 8, 48, 3, depth, None, 8, 8, 48, None, None, 32, 1, 0, bv) == _abi.E_INVALID
    assert product_lib.v1c_build_ftab(_abi.INTER_CUBIC, None) == _abi.E_INVALID
    assert product_lib.v1c_build_ftab(_abi.INTER_NEAREST, (C.c_float * 16)()) == _abi.E_INVALID
    # 16U pitches are bytes: a row of 8 BGR uint16 pixels is 48 bytes, an odd pitch is refused before any device work
    assert product_lib.v1c_remap_lut_ex(0, None, C.c_void_p(4096), 8, 8, 47, 3, 2, C.c_void_p(8192), 8, 8, 48, C.c_void_p(4),
                                        C.c_void_p(4), 32, 1, 0, bv) == _abi.E_INVALID


@pytest.mark.parametrize("dtype", [np.float64, np.int16, np.int8])
def test_other_numpy_types_raise(dtype):
    from vr180_convert_amd import remapper

    with pytest.raises(TypeError):
        remapper._to_device(np.zeros((4, 4, 3), dtype), None)


def test_mixed_src_dst_types_raise():
    import torch

    from vr180_convert_amd import remapper

    src = torch.zeros((8, 8, 3), dtype=torch.uint16)
    dst = torch.zeros((8, 8, 3), dtype=torch.float32)
    with pytest.raises(TypeError):
        remapper.marshal_units([src], [dst], None, src_hw=(8, 8), dst_wh=(8, 8), cn=3, device=None)
    with pytest.raises(TypeError):
        remapper.remap_tensors(None, [src], [dst], radius=4.0)
    with pytest.raises(TypeError):
        remapper._check_image_tensor(torch.zeros((8, 8, 3), dtype=torch.int16), "src")


def decode_png(data: bytes):
    """A few lines of PNG reading: IHDR, the concatenated IDAT stream, scanline filters 0 - 4."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, {}
    idat = b""
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        pos += 12 + n
        chunks[kind] = body
        if kind == b"IDAT":
            idat += body
    w, h, depth, ctype = struct.unpack(">IIBB", chunks[b"IHDR"][:10])
    cn = {0: 1, 2: 3, 6: 4}[ctype]
    bpp = cn * depth // 8
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * bpp)
    out = np.zeros((h, w * bpp), np.int64)
    prev = np.zeros(w * bpp, np.int64)
    for r in range(h):
        f, line = raw[r, 0], raw[r, 1:].astype(np.int64)
        cur = np.zeros_like(line)
        for i in range(len(line)):
            a = cur[i - bpp] if i >= bpp else 0
            b, c = prev[i], (prev[i - bpp] if i >= bpp else 0)
            if f == 4:  # Paeth
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            else:
                pred = [0, a, b, (a + b) // 2][f]
            cur[i] = (line[i] + pred) & 255
        out[r], prev = cur, cur
    px = out.astype(np.uint8).reshape(h, w * bpp)
    if depth == 16:
        px = px.view(">u2").astype(np.uint16)
    return depth, px.reshape(h, w, cn)


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_png16_round_trip(tmp_path, cn):
    from vr180_convert_amd import _io

    rng = np.random.default_rng(cn)
    img = rng.integers(0, 65536, (21, 17, cn)).astype(np.uint16)
    img[0, 0] = 0x1234  # byte order shows
    p = tmp_path / "x.png"
    assert _io.imwrite(p, img if cn > 1 else img[..., 0])
    depth, px = decode_png(p.read_bytes())
    assert depth == 16
    want = img if cn == 1 else img[..., [2, 1, 0] + ([3] if cn == 4 else [])]  # PNG order RGB(A)
    assert np.array_equal(px, want)


def test_npy_keeps_type_and_float_png_saturates(tmp_path):
    from vr180_convert_amd import _io

    # other types (the float64 anaglyph of merge=True) are saturated to uint8 in .npy as before
    _io.imwrite(tmp_path / "g.npy", np.array([[[-1.0, 2.5, 300.0]]]))
    g = np.load(tmp_path / "g.npy")
    assert g.dtype == np.uint8 and list(g[0, 0]) == [0, 2, 255]
    h = np.array([[[1.5, 70000.0, -2.0]]], np.float32)
    _io.imwrite(tmp_path / "h.npy", h)
    assert np.array_equal(np.load(tmp_path / "h.npy"), h)

    a = np.arange(12, dtype=np.uint16).reshape(2, 2, 3) * 1000
    _io.imwrite(tmp_path / "a.npy", a)
    b = np.load(tmp_path / "a.npy")
    assert b.dtype == np.uint16 and np.array_equal(a, b)
    f = np.array([[[-1.0, 2.5, 300.0]]], np.float32)
    _io.imwrite(tmp_path / "f.png", f)
    depth, px = decode_png((tmp_path / "f.png").read_bytes())
    assert depth == 8 and list(px[0, 0]) == [255, 2, 0]  # rint + saturate, then BGR -> RGB


def test_wide_kernels_use_no_scratch(tmp_path, product_lib):
    from test_resource_budget import CSRC, kernel_metadata

    ks = kernel_metadata(tmp_path, CSRC / "kernels_wide.o")
    assert len(ks) == 2 * 3 * 4 * 4  # {u16, f32} x cn {1, 3, 4} x 4 interpolations x 4 coordinate modes
    bad = [(k[".name"], k[".private_segment_fixed_size"], k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for k in ks
           if k[".private_segment_fixed_size"] or k[".sgpr_spill_count"] or k[".vgpr_spill_count"]]
    # MODE_LITERAL (0) / MODE_FIXUP (3) carry the fp64 interpreter: the allowance test_resource_budget.py gives k_remap
    bad = [b for b in bad if not b[0].endswith(("Li0EEEvNS_9KernelCtxENS_8UnitArgsENS_8WideArgsE",
                                                "Li3EEEvNS_9KernelCtxENS_8UnitArgsENS_8WideArgsE"))]
    assert not bad, bad


@pytest.mark.parametrize("fn", ["auto_radius_tensor", "anaglyph_tensors"])
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_byte_kernels_refuse_wide_tensors(fn, dtype):
    """get_radius's and the anaglyph's device kernels read bytes: wide tensors raise before anything is launched."""
    import torch

    from vr180_convert_amd import remapper

    t = torch.zeros((8, 8, 3), dtype=getattr(torch, dtype))
    with pytest.raises(TypeError):
        if fn == "auto_radius_tensor":
            remapper.auto_radius_tensor([t])
        else:
            remapper.anaglyph_tensors(t, t)


class _FakePlan:
    """Stands in for a device plan: validates its units as Plan.run does (marshal_units, host tensors)."""

    def __init__(self, kw):
        self.kw, self.path, self.runs = kw, "ray", []

    def run(self, srcs, dsts, rots):
        from vr180_convert_amd import remapper

        remapper.marshal_units(srcs, dsts, rots, src_hw=self.kw["src_hw"], dst_wh=self.kw["dst_wh"], cn=self.kw["cn"], device=None,
                               dtype=self.kw["dtype"])
        self.runs.append([s.dtype for s in srcs])

    def last_launch(self):
        return "wide"


def test_shared_plan_memo_keys_every_unit(monkeypatch):
    """remap_tensors' shortcut to the previous call's plan must not take a call whose units differ in type or shape from that call's."""
    import torch

    from vr180_convert_amd import remapper
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder, PolynomialScaler

    plans = {}

    def plan_for(chain, **kw):
        return plans.setdefault((bytes(chain), kw["src_hw"], kw["dtype"]), _FakePlan(kw))

    monkeypatch.setattr(remapper, "_plan_for", plan_for)
    remapper.clear_caches()
    t = EquirectangularEncoder() * PolynomialScaler([0, 1, -0.1]) * FisheyeDecoder("equidistant")
    u16 = [torch.zeros((16, 16, 3), dtype=torch.uint16) for _ in range(2)]
    f32 = [torch.zeros((16, 16, 3), dtype=torch.float32) for _ in range(2)]
    odd = torch.zeros((16, 17, 3), dtype=torch.uint16)
    kw = dict(radius=8.0, interpolation=1, size_input=(16, 16))
    try:
        remapper.remap_tensors(t, [u16[0]], [u16[1]], **kw)
        remapper.remap_tensors(t, [u16[0]], [u16[1]], **kw)  # (the shortcut)
        remapper.remap_tensors(t, [u16[0], f32[0]], [u16[1], f32[1]], **kw)  # one plan per type
        remapper.remap_tensors(t, [u16[0], odd], [u16[1], torch.zeros((16, 16, 3), dtype=torch.uint16)], **kw)  # one plan per shape
        remapper.remap_tensors(t, [u16[0]], [u16[1]], **kw)
    finally:
        remapper.clear_caches()
    assert len(plans) == 3
    assert sorted(len(p.runs) for p in plans.values()) == [1, 1, 5]


# ---- the adversarial cases the GPU half runs (tests/wide_cases.py): generators and restatement proven on the host first ------------
@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("interp", [0, 1, 2, 3, 4])
def test_wide_cases_host_sampler_equals_restatement(product_lib, wide_emul, dtype, interp):
    """Special-valued maps, 1-pixel sources, pitched and odd-offset views, extreme float32 pixels: the whole buffers are compared, so a
    store outside the destination view shows as well."""
    import wide_cases as WC

    ftab = product_ftab(product_lib, interp) if interp in (R.INTER_CUBIC, R.INTER_LANCZOS4) else None
    n = 0
    for c in WC.cases(dtype, interp):
        sbuf = WC.place(c.src_view, c.src)
        dbuf = WC.place(c.dst_view, c.fill)
        want = dbuf.copy()
        WC.window(c.dst_view, want, c.fill.shape)[...] = R.remap(c.src, c.xm, c.ym, c.interp, c.border, c.bv, dst=c.fill)
        cval = product_cval(wide_emul, DEPTH[dtype], c.bv)
        isz = sbuf.dtype.itemsize
        hs, ws, cn = c.src.shape
        ho, wo = c.xm.shape
        rc = wide_emul.wide_remap_host(sbuf.ctypes.data + c.src_view.offset * isz, hs, ws, c.src_view.pitch * isz, cn, DEPTH[dtype],
                                       dbuf.ctypes.data + c.dst_view.offset * isz, ho, wo, c.dst_view.pitch * isz, c.xm.ctypes.data,
                                       c.ym.ctypes.data, c.interp, c.border, cval.ctypes.data, None if ftab is None else ftab.ctypes.data)
        assert rc == 0
        assert WC.same(dbuf, want), (str(c), WC.ndiff(dbuf, want))
        n += 1
    assert n == 6 * 3 * WC.ROUNDS


def test_wide_cases_cover_what_they_are_for():
    import test_gpu_wide
    import wide_cases as WC

    assert all(v in WC.BORDER_VALUES for v in test_gpu_wide.BVS)
    for dtype in WC.DTYPES:
        for interp in WC.INTERPS:
            cs = list(WC.cases(dtype, interp))
            assert {(c.border, c.cn) for c in cs} == {(b, n) for b in WC.BORDERS for n in WC.CNS}
            assert {c.xm.shape[1] for c in cs} == set(WC.OUT_WIDTHS) and {c.xm.shape[0] for c in cs} == set(WC.OUT_HEIGHTS)
            assert {c.dst_view.kind for c in cs} == set(WC.VIEWS) and {c.src_view.kind for c in cs} == set(WC.VIEWS)
            assert {c.src_kind for c in cs} == set(WC.SRC_KINDS) and {c.map_kind for c in cs} == set(WC.MAP_KINDS)
            assert {c.map_pad for c in cs} == set(WC.MAP_PADS)
            if dtype == np.uint16:
                # a destination row that is 2-byte aligned only -- by the view's offset, and by an odd pitch behind an aligned offset
                # -- under a full lane (4 pixels written), for cn 1 and 3 (cn 4: an odd offset alone does it)
                odd = [c for c in cs if c.dst_view.kind == "pitched-odd" and c.xm.shape[1] >= 4]
                assert {c.cn for c in odd} == {1, 3, 4}
                assert any(c.dst_view.pitch % 2 for c in cs if c.cn in (1, 3) and c.xm.shape[0] > 1)
            else:
                ext = [c for c in cs if c.extremes]
                assert len(cs) // 4 <= len(ext) <= len(cs) // 2
                px = np.concatenate([c.src.reshape(-1) for c in ext])
                assert np.isnan(px).any() and np.isinf(px).any() and (np.abs(px) > 3e38).any() and (np.signbit(px) & (px == 0)).any()
                assert ((px != 0) & (np.abs(px) < np.float32(1.1754944e-38))).any()  # denormals
    a, b = list(WC.cases(np.float32, 4)), list(WC.cases(np.float32, 4))
    assert all(np.array_equal(x.xm, y.xm, equal_nan=True) and np.array_equal(x.src, y.src, equal_nan=True) for x, y in zip(a, b))
