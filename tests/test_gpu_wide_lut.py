"""k_remap_wide on the MI355X under adversarial inputs (tests/wide_cases.py): special-valued maps, 1-pixel sources, output sizes either
side of the lane's 4 pixels and the workgroup's 256 x 4 block, pitched views whose destination is 2-byte aligned only, float32
denormals / values next to FLT_MAX / signed zeros -- v1c_remap_lut_ex by ctypes, remap_tensors with a user-defined transformer, a
lowered chain on the same views and a batch split in two launches, each against the NumPy restatement (wide_ref.py), byte for byte
(float32: equal, NaN <=> NaN).  Whole buffers are compared: a store outside the destination view fails the test as well.
tests/test_wide_host.py runs the same cases through the host build of the sampler."""
import numpy as np
import pytest
import torch

import chainspecs as CS
import wide_cases as WC
import wide_ref as W

pytestmark = pytest.mark.gpu

DEPTH = {np.uint16: 2, np.float32: 5}
RAY = [("equirect_enc", True), ("poly", [0, 1, -0.1]), CS.EQUI]


@pytest.fixture(scope="module")
def lib():
    from vr180_convert_amd import _native

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    return _native.lib()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def lut_ex(lib, dev, c):
    """one case through v1c_remap_lut_ex: (the destination buffer after the call, what it must hold)"""
    from vr180_convert_amd import _native
    from vr180_convert_amd.remapper import _stream_ptr, border_scalar_f64

    hs, ws, cn = c.src.shape
    ho, wo = c.xm.shape
    sbuf, dbuf = WC.place(c.src_view, c.src), WC.place(c.dst_view, c.fill)
    want = dbuf.copy()
    WC.window(c.dst_view, want, c.fill.shape)[...] = W.remap(c.src, c.xm, c.ym, c.interp, c.border, c.bv, dst=c.fill)
    xw, yw = np.full((ho, wo + c.map_pad), np.nan, np.float32), np.full((ho, wo + c.map_pad), np.nan, np.float32)
    xw[:, :wo], yw[:, :wo] = c.xm, c.ym
    s_d, d_d = torch.from_numpy(sbuf).to(dev), torch.from_numpy(dbuf).to(dev)
    x_d, y_d = torch.from_numpy(xw).to(dev), torch.from_numpy(yw).to(dev)
    isz = sbuf.dtype.itemsize
    bv = border_scalar_f64(c.bv)
    rc = lib.v1c_remap_lut_ex(dev.index, _stream_ptr(dev), s_d.data_ptr() + c.src_view.offset * isz, hs, ws, c.src_view.pitch * isz, cn,
                              DEPTH[c.dtype], d_d.data_ptr() + c.dst_view.offset * isz, ho, wo, c.dst_view.pitch * isz, x_d.data_ptr(),
                              y_d.data_ptr(), (wo + c.map_pad) * 4, c.interp, c.border, bv.ctypes.data)
    _native.check(rc, "v1c_remap_lut_ex")
    return d_d.cpu().numpy(), want


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("interp", [0, 1, 2, 3, 4])
def test_lut_ex_on_adversarial_cases(lib, dev, dtype, interp):
    n = 0
    for c in WC.cases(dtype, interp):
        got, want = lut_ex(lib, dev, c)
        assert WC.same(got, want), (str(c), WC.ndiff(got, want))
        n += 1
    assert n == 6 * 3 * WC.ROUNDS


def strided(dev, view, img):
    """(flat device buffer, the image as a strided view of it)"""
    h, w, cn = img.shape
    buf = torch.from_numpy(WC.place(view, img)).to(dev)
    return buf, torch.as_strided(buf, (h, w, cn), (view.pitch, cn, 1), view.offset)


def odd_views(dtype, hs, ws, ho, wo, cn, seed, extremes=False):
    rng = np.random.default_rng(seed)
    src = WC.draw_pixels(rng, dtype, (hs, ws, cn), extremes)
    fill = WC.draw_pixels(rng, dtype, (ho, wo, cn))
    return src, fill, WC.draw_view(rng, "pitched-odd", hs, ws, cn, dtype), WC.draw_view(rng, "pitched-odd", ho, wo, cn, dtype)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_user_transformer_on_pitched_odd_offset_views(lib, dev, dtype):
    """remap_tensors -> v1c_remap_lut_ex with the strides of real views; the transformer sends part of the image to NaN and far outside"""
    import vr180_convert_amd as V
    from vr180_convert_amd import remapper as R
    from vr180_convert_amd.chain import TransformerBase

    class Torn(TransformerBase):
        def transform(self, x, y, **kwargs):
            with np.errstate(divide="ignore", invalid="ignore"):
                # (normalised by half the output's smaller side: x spans +-29 for the 261 x 9 output below)
                return np.where(np.abs(x) < 0.3, np.nan, 0.05 * x + 0.15 * y), np.where(y > 0.5, y / (1.0 - y), y * 0.95) * np.where(x > 25, 1e30, 1.0)

        def inverse_transform(self, x, y, **kwargs):
            return x, y

    t = Torn()
    for k, (cn, interp, border) in enumerate(((3, 4, 4), (1, 1, 5), (4, 2, 0), (3, 0, 3))):
        src, fill, sv, dv = odd_views(dtype, 40, 33, 9, 261, cn, (5, k), extremes=True)
        sbuf, s = strided(dev, sv, src)
        dbuf, d = strided(dev, dv, fill)
        bv = WC.BORDER_VALUES[k + 1]
        V.remap_tensors(t, [s], [d], radius=17.0, interpolation=interp, boarder_mode=border, boarder_value=bv)
        torch.cuda.synchronize()
        assert R.last_launch_kinds() == ["lut"]
        xm, ym = R._host_map(t, radius=17.0, size_input=(40, 33), size_output=(261, 9))
        assert np.isnan(xm).any() and (np.abs(ym) > 1e20).any()
        want = WC.place(dv, fill)
        WC.window(dv, want, fill.shape)[...] = W.remap(src, xm, ym, interp, border, bv, dst=fill)
        got = dbuf.cpu().numpy()
        assert WC.same(got, want), (dtype, cn, interp, border, WC.ndiff(got, want))


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_lowered_chain_on_pitched_odd_offset_views(lib, dev, oracle_mod, dtype):
    """the ray path (k_remap_wide behind a plan) storing through a destination that is 2-byte aligned only"""
    import vr180_convert_amd as V
    from vr180_convert_amd import remapper as R

    for k, (cn, interp, border) in enumerate(((3, 1, 0), (1, 4, 5), (4, 2, 1))):
        src, fill, sv, dv = odd_views(dtype, 96, 104, 70, 261, cn, (6, k), extremes=True)
        sbuf, s = strided(dev, sv, src)
        dbuf, d = strided(dev, dv, fill)
        bv = WC.BORDER_VALUES[k]
        V.remap_tensors(CS.to_product(RAY), [s], [d], radius=48.0, interpolation=interp, boarder_mode=border, boarder_value=bv)
        torch.cuda.synchronize()
        kinds = R.last_launch_kinds()
        assert kinds in (["wide"], ["wide+fixup"]), kinds
        xm, ym = oracle_mod.get_map(RAY, radius=48.0, size_input=(96, 104), size_output=(261, 70))
        want = WC.place(dv, fill)
        WC.window(dv, want, fill.shape)[...] = W.remap(src, xm, ym, interp, border, bv, dst=fill)
        got = dbuf.cpu().numpy()
        assert WC.same(got, want), (dtype, cn, interp, border, WC.ndiff(got, want))


def test_seventeen_float32_units_with_extremes(lib, dev, oracle_mod):
    """a batch split in two launches (16 + 1 units): the second launch's unit holds the extreme values too"""
    import vr180_convert_amd as V
    from vr180_convert_amd import remapper as R

    n = 17
    rng = np.random.default_rng(9)
    srcs = [WC.draw_pixels(rng, np.float32, (64, 72, 3), extremes=True) for _ in range(n)]
    fill = WC.draw_pixels(rng, np.float32, (50, 57, 3))
    s = [torch.from_numpy(a).to(dev) for a in srcs]
    d = [torch.from_numpy(fill.copy()).to(dev) for _ in range(n)]
    V.remap_tensors(CS.to_product(RAY), s, d, radius=32.0, interpolation=2, boarder_mode=5, boarder_value=(1e-40, 3e38, -1))
    torch.cuda.synchronize()
    assert R.last_launch_kinds()[0].startswith("wide")
    xm, ym = oracle_mod.get_map(RAY, radius=32.0, size_input=(64, 72), size_output=(57, 50))
    for k in range(n):
        assert (np.abs(srcs[k]) > 3e38).any() and ((srcs[k] != 0) & (np.abs(srcs[k]) < 1e-38)).any()
        want = W.remap(srcs[k], xm, ym, 2, 5, (1e-40, 3e38, -1), dst=fill)
        got = d[k].cpu().numpy()
        assert WC.same(got, want), (k, WC.ndiff(got, want))
