"""NumPy restatement of the lossless JPEG composer's contract: rotation, flip and transpose of rectangles of
MCUs in the DCT domain, gathered from up to four files into one output.  What a single file is taken for, the output's geometry, the
header writer and the entropy coder are the transcoder's restatement's (jpgxc_ref) and through it the codecs' (jpg_ref, jpg_opt_ref,
jpgdec_ref): nothing of them is restated here.

A transform is three bits -- 4: transpose first, 1: then mirror x, 2: then mirror y.  With F[v][u] a block's coefficient of vertical
frequency v and horizontal frequency u, the transpose gives F'[v][u] = F[u][v], mirror x multiplies by (-1)^u, mirror y by (-1)^v.
The MCUs of a region and the luma blocks of an MCU move the same way.

An output is ``{"width", "height", "regions": [(source, transform, src_x, src_y, nx, ny, dst_x, dst_y), ...]}`` with the regions in
MCUs and the transform a name or a code, and optionally ``"restart_mcus"`` (None: one MCU row; 0: no restart markers) and
``"optimize"``."""
from __future__ import annotations

import copy

import numpy as np

import jpg_opt_ref as O
import jpg_ref as R
import jpgxc_ref as X
from jpgxc_ref import Invalid, Source, Unsupported  # noqa: F401

MAX_SOURCES = 4
MAX_REGIONS = 16
MAX_OUTPUTS = 16

TRANSFORMS = {"none": 0, "flip_h": 1, "flip_v": 2, "rot180": 3, "transpose": 4, "rot90": 5, "rot270": 6, "transverse": 7}
NAMES = {v: k for k, v in TRANSFORMS.items()}
INVERSE = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 5, 7: 7}
MIRROR_X, MIRROR_Y, TRANSPOSE = 1, 2, 4

_NATURAL = np.arange(64).reshape(8, 8)
_POS = np.argsort(R.ZIGZAG)                      # zigzag position of a row-major index
TZ = _POS[_NATURAL.T.reshape(64)[R.ZIGZAG]]      # zigzag position of the transposed place of a zigzag position
SIGN_X = np.where(R.ZIGZAG % 2, -1, 1)           # (-1)^u over the zigzag order
SIGN_Y = np.where(R.ZIGZAG // 8 % 2, -1, 1)      # (-1)^v


def code_of(transform) -> int:
    if isinstance(transform, str):
        if transform not in TRANSFORMS:
            raise Invalid(f"no transform {transform!r}")
        return TRANSFORMS[transform]
    if transform is None:
        return 0
    if not 0 <= int(transform) <= 7:
        raise Invalid("a transform's code is 0 ... 7")
    return int(transform)


def placed(code, nx, ny):
    """the MCUs a region of nx x ny source MCUs covers in the output"""
    return (ny, nx) if code & TRANSPOSE else (nx, ny)


def transform_mcus(mcus, code, hs, vs):
    """(ny, nx, bpm, 64) MCUs -- any integer type -- transformed: (NY, NX, bpm, 64)"""
    luma = hs * vs
    y, c = mcus[:, :, :luma], mcus[:, :, luma:]
    y = y.reshape(y.shape[0], y.shape[1], vs, hs, 64)
    if code & TRANSPOSE:
        y, c = y.transpose(1, 0, 3, 2, 4)[..., TZ], c.transpose(1, 0, 2, 3)[..., TZ]
    if code & MIRROR_X:
        y, c = y[:, ::-1, :, ::-1] * SIGN_X, c[:, ::-1] * SIGN_X
    if code & MIRROR_Y:
        y, c = y[::-1, :, ::-1] * SIGN_Y, c[::-1] * SIGN_Y
    return np.concatenate([y.reshape(y.shape[0], y.shape[1], luma, 64), c], axis=2)


def effective_tables(src: Source, code):
    """the quantisation tables a region's blocks are read with: [luminance, chrominance] row-major, transposed where it transposes"""
    s = src.info
    tabs = [np.asarray(s.q[s.tq[0]]), np.asarray(s.q[s.tq[1 if s.nc == 3 else 0]])]
    return [t.reshape(8, 8).T.reshape(64) if code & TRANSPOSE else t for t in tabs]


def sources_of(datas) -> list:
    if not 1 <= len(datas) <= MAX_SOURCES:
        raise Invalid("1 ... 4 sources")
    srcs = [d if isinstance(d, Source) else Source(d) for d in datas]
    a = srcs[0].info
    for s in srcs[1:]:
        if (s.info.nc, s.info.hs, s.info.vs) != (a.nc, a.hs, a.vs):
            raise Unsupported("sources of different components or sampling factors")
    return srcs


def check(srcs, out: dict) -> R.Geom:
    """the rules of one output; returns its geometry"""
    g = X.geom(srcs[0], out["width"], out["height"], out.get("restart_mcus"))
    regs = out["regions"]
    if not 1 <= len(regs) <= MAX_REGIONS:
        raise Invalid("1 ... 16 regions")
    covered = np.zeros((g.mcuy, g.mcux), np.int64)
    overlap = False
    for n, (si, tr, sx, sy, nx, ny, dx, dy) in enumerate(regs):
        if not 0 <= si < len(srcs):
            raise Invalid("no such source")
        code = code_of(tr)
        s = srcs[si].info
        if min(sx, sy, dx, dy) < 0 or nx < 1 or ny < 1:
            raise Invalid("negative origin or empty region")
        if sx + nx > s.mcux or sy + ny > s.mcuy:
            raise Invalid("a region leaves its source")
        if code & TRANSPOSE and s.hs != s.vs:
            raise Unsupported("a transposed 4:2:2 file would be 4:4:0")
        NX, NY = placed(code, nx, ny)
        if dx + NX > g.mcux or dy + NY > g.mcuy:
            raise Invalid("a region leaves the output")
        if covered[dy:dy + NY, dx:dx + NX].any():
            raise Unsupported("regions overlap in the output")
        covered[dy:dy + NY, dx:dx + NX] += 1
        if n and not all(np.array_equal(a, b) for a, b in zip(effective_tables(srcs[si], code), effective_tables(srcs[regs[0][0]], code_of(regs[0][1])))):
            raise Unsupported("a region's effective quantisation tables are not region 0's")
    if covered.min() < 1:
        raise Invalid("an MCU of the output is uncovered")
    return g


def gather(srcs, out: dict, g: R.Geom) -> np.ndarray:
    """the output's (nblocks, 64) coefficients"""
    a = srcs[0].info
    dst = np.zeros((g.mcuy, g.mcux, a.bpm, 64), np.int64)
    dc = np.zeros((g.mcuy, g.mcux, a.bpm), np.int64)
    for si, tr, sx, sy, nx, ny, dx, dy in out["regions"]:
        code, src = code_of(tr), srcs[si]
        s = src.info
        mcus = src.coef.reshape(s.mcuy, s.mcux, s.bpm, 64)[sy:sy + ny, sx:sx + nx].astype(np.int64)
        NX, NY = placed(code, nx, ny)
        moved = transform_mcus(mcus, code, s.hs, s.vs)
        dst[dy:dy + NY, dx:dx + NX] = moved
        # the DC before it is cut to 16 bits goes where its block goes (no transform changes a DC)
        sums = np.zeros(mcus.shape, np.int64)
        sums[..., 0] = src.dc.reshape(s.mcuy, s.mcux, s.bpm)[sy:sy + ny, sx:sx + nx]
        dc[dy:dy + NY, dx:dx + NX] = transform_mcus(sums, code, s.hs, s.vs)[..., 0]
    if np.abs(dst[..., 1:]).max(initial=0) > 1023 or dc.min() < -1024 or dc.max() > 1023:
        raise Unsupported("a gathered coefficient outside what 8-bit samples give")
    return dst.astype(np.int16).reshape(-1, 64)


def header_source(srcs, out: dict) -> Source:
    """the source whose tables and sampling factors the output's header carries: region 0's, its tables transposed where region 0 transposes"""
    si, tr = out["regions"][0][:2]
    src = srcs[si]
    if not code_of(tr) & TRANSPOSE:
        return src
    shim = copy.copy(src)
    shim.info = copy.copy(src.info)
    q = src.info.q
    keys = q.keys() if isinstance(q, dict) else range(len(q))
    tq = {k: (np.asarray(q[k]).reshape(8, 8).T.reshape(64) if q[k] is not None else None) for k in keys}
    shim.info.q = tq if isinstance(q, dict) else [tq[k] for k in keys]
    return shim


def parts(srcs, out: dict):
    """(coefficients, header, scan) of one output"""
    g = check(srcs, out)
    zz = gather(srcs, out, g)
    hs = header_source(srcs, out)
    if out.get("optimize"):
        specs = O.tables(zz, g)
        return zz, X.headers(hs, g, specs), O.scan(zz, g, specs)
    return zz, X.headers(hs, g), R.scan(zz, g)


def compose(datas, outputs) -> list:
    """every output's file"""
    srcs = sources_of(datas)
    if not 1 <= len(outputs) <= MAX_OUTPUTS:
        raise Invalid("1 ... 16 outputs")
    files = []
    for o in outputs:
        _, head, scan = parts(srcs, o)
        files.append(head + scan + b"\xff\xd9")
    return files


# ---- the uses, in pixels (vr180_convert_amd/jpeg_compose_device.py) ---------------------------------------------------------------------
def transformed_size(src: Source, code, trim=False):
    """(width, height, nx, ny) of the whole image under a transform: the pixel size of the result and the source MCUs it takes.  A
    mirrored axis must be whole MCUs (ValueError) unless ``trim`` cuts the partial last column or row off first."""
    s = src.info
    w, h = s.w, s.h
    mirrored_w = bool(code & (MIRROR_Y if code & TRANSPOSE else MIRROR_X))  # (a mirror after the transpose mirrors the source's other axis)
    mirrored_h = bool(code & (MIRROR_X if code & TRANSPOSE else MIRROR_Y))
    if mirrored_w and w % src.mw:
        if not trim or w < src.mw:
            raise ValueError("width")
        w -= w % src.mw
    if mirrored_h and h % src.mh:
        if not trim or h < src.mh:
            raise ValueError("height")
        h -= h % src.mh
    nx, ny = -(-w // src.mw), -(-h // src.mh)
    return (h, w, nx, ny) if code & TRANSPOSE else (w, h, nx, ny)


def transform_output(src: Source, transform, trim=False, **kw) -> dict:
    code = code_of(transform)
    w, h, nx, ny = transformed_size(src, code, trim)
    return dict(width=w, height=h, regions=[(0, code, 0, 0, nx, ny, 0, 0)], **kw)


def transform_jpeg(data, op, *, trim=False, optimize=False, restart_mcus=None) -> bytes:
    src = Source(data)
    return compose([src], [transform_output(src, op, trim, optimize=optimize, restart_mcus=restart_mcus)])[0]


def join_output(left: Source, right: Source, left_transform=None, right_transform=None, trim=False, **kw) -> dict:
    lc, rc = code_of(left_transform), code_of(right_transform)
    lw, lh, lnx, lny = transformed_size(left, lc, trim)
    rw, rh, rnx, rny = transformed_size(right, rc, trim)
    mw = left.mh if lc & TRANSPOSE else left.mw
    if lw % mw:
        if not trim or lw < mw:
            raise ValueError("the left eye's width")
        lw -= lw % mw
        if lc & TRANSPOSE:
            lny = lw // mw
        else:
            lnx = lw // mw
    if lh != rh:
        raise ValueError("heights")
    NX = placed(lc, lnx, lny)[0]
    return dict(width=lw + rw, height=lh, regions=[(0, lc, 0, 0, lnx, lny, 0, 0), (1, rc, 0, 0, rnx, rny, NX, 0)], **kw)


def join_sbs_jpeg(left, right, *, left_transform=None, right_transform=None, trim=False, optimize=False, restart_mcus=None) -> bytes:
    l, r = Source(left), Source(right)
    return compose([l, r], [join_output(l, r, left_transform, right_transform, trim, optimize=optimize, restart_mcus=restart_mcus)])[0]
