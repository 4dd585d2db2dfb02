"""NumPy restatement of the lossless JPEG transcoder's contract: which files are taken, the rules of an
output's regions, the gathered coefficients, and the output's file -- the FILE's quantisation tables and sampling factors around the
encoder's entropy coding of the gathered coefficients.  The coefficients are the decoder's restatement's (jpgdec_ref), the entropy
coder, the optimised tables and the segments are the encoder's (jpg_ref, jpg_opt_ref): nothing of them is restated here.

An output is ``{"width", "height", "regions": [(src_x, src_y, nx, ny, dst_x, dst_y), ...]}`` with the regions in MCUs, and optionally
``"restart_mcus"`` (None: one MCU row; 0: no restart markers) and ``"optimize"``."""
from __future__ import annotations

import struct

import numpy as np

import jpg_opt_ref as O
import jpg_ref as R
import jpgdec_ref as D

MAX_REGIONS = 16
MAX_OUTPUTS = 16


class Unsupported(Exception):
    """V1C_E_UNSUPPORTED"""


class Invalid(Exception):
    """V1C_E_INVALID"""


class Source:
    """a file as the transcoder sees it: the parse, and (nblocks, 64) coefficients in zigzag order, MCU-major, the DC a value"""

    def __init__(self, data):
        try:
            d = D.decode(data, check=False)
        except D.Unsupported as e:
            raise Unsupported(str(e)) from e
        s = self.info = d.info
        if s.nc == 3 and not np.array_equal(s.q[s.tq[1]], s.q[s.tq[2]]):
            raise Unsupported("more than two classes of quantisation tables")
        self.coef = D.dc_values(s, d.coef)
        self.dc = _dc_sums(s, d.coef)  # the DC values before they are cut to 16 bits: what the range rule judges
        self.mw, self.mh = 8 * s.hs, 8 * s.vs


def _dc_sums(s, coef):
    """every block's DC as the sum of its component's differences from the block's restart segment on, in 64 bits (jpgdec_ref.dc_values
    gives the same cut to 16 bits, which is what a decoder shows)"""
    b = np.arange(s.nblocks)
    mcu, k = b // s.bpm, b % s.bpm
    out = np.zeros(s.nblocks, np.int64)
    d = coef[:, 0].astype(np.int64)
    comp = np.where(k < s.ny, 0, k - s.ny + 1)
    seg = mcu // s.interval
    for c in range(s.nc):
        idx = np.nonzero(comp == c)[0]
        total = np.cumsum(d[idx])
        first = np.concatenate([[True], seg[idx][1:] != seg[idx][:-1]])
        base = np.maximum.accumulate(np.where(first, np.arange(len(idx)), 0))
        out[idx] = total - (total[base] - d[idx][base])
    return out


def geom(src: Source, width, height, restart_mcus) -> R.Geom:
    """the encoder's geometry of an output; restart_mcus: None (one MCU row), 0 (one interval: no markers) or 1 ... 65535"""
    s = src.info
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise Invalid("size")
    g = R.Geom(height, width, 1 if s.nc == 1 else 3, "420" if (s.hs, s.vs) == (2, 2) else "444", 1)
    if (s.hs, s.vs) == (2, 1):  # 4:2:2, which the encoder's restatement does not write itself: MCUs of 16 x 8 pixels, Y Y Cb Cr
        g.bpm, g.comp = 4, np.array([0, 0, 1, 2])
        g.mcux, g.mcuy = -(-width // 16), -(-height // 8)
        g.nmcu = g.mcux * g.mcuy
        g.nblocks = g.nmcu * g.bpm
    r = g.mcux if restart_mcus is None else int(restart_mcus)
    if not 0 <= r <= 65535:
        raise Invalid("restart_mcus")
    g.restart = r or g.nmcu
    g.nint = -(-g.nmcu // g.restart)
    g.dri = r
    return g


def check(src: Source, out: dict) -> R.Geom:
    """the rules of one output; returns its geometry"""
    s = src.info
    g = geom(src, out["width"], out["height"], out.get("restart_mcus"))
    regs = out["regions"]
    if not 1 <= len(regs) <= MAX_REGIONS:
        raise Invalid("1 ... 16 regions")
    covered = np.zeros((g.mcuy, g.mcux), np.int64)
    for sx, sy, nx, ny, dx, dy in regs:
        if min(sx, sy, dx, dy) < 0 or nx < 1 or ny < 1:
            raise Invalid("negative origin or empty region")
        if sx + nx > s.mcux or sy + ny > s.mcuy:
            raise Invalid("a region leaves the source")
        if dx + nx > g.mcux or dy + ny > g.mcuy:
            raise Invalid("a region leaves the output")
        covered[dy:dy + ny, dx:dx + nx] += 1
    if covered.max() > 1:
        raise Unsupported("regions overlap in the output")
    if covered.min() < 1:
        raise Invalid("an MCU of the output is uncovered")
    return g


def gather(src: Source, out: dict, g: R.Geom) -> np.ndarray:
    """the output's (nblocks, 64) coefficients: every MCU of every region, as it is"""
    s = src.info
    mcus = src.coef.reshape(s.mcuy, s.mcux, s.bpm, 64)
    dcs = src.dc.reshape(s.mcuy, s.mcux, s.bpm)
    dst = np.zeros((g.mcuy, g.mcux, s.bpm, 64), np.int16)
    dc = np.zeros((g.mcuy, g.mcux, s.bpm), np.int64)
    for sx, sy, nx, ny, dx, dy in out["regions"]:
        dst[dy:dy + ny, dx:dx + nx] = mcus[sy:sy + ny, sx:sx + nx]
        dc[dy:dy + ny, dx:dx + nx] = dcs[sy:sy + ny, sx:sx + nx]
    # the range rule, over the GATHERED blocks only: what the cut leaves out is not coded again and does not matter
    if np.abs(dst[..., 1:]).max(initial=0) > 1023 or dc.min() < -1024 or dc.max() > 1023:
        raise Unsupported("a gathered coefficient outside what 8-bit samples give")
    return dst.reshape(-1, 64)


def headers(src: Source, g: R.Geom, specs=None) -> bytes:
    """SOI, APP0 (JFIF 1.01, aspect 1:1), DQT with the file's tables as 0 and 1, SOF0 (SOF1 and 16-bit tables where an entry passes 255)
    with the file's sampling factors, DHT (``specs`` of an optimising output, else Annex K), DRI unless there are no restart markers,
    SOS"""
    s = src.info
    out = b"\xff\xd8" + R._segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    tabs = [s.q[s.tq[0]]] + ([s.q[s.tq[1]]] if s.nc == 3 else [])
    wide = any(int(t.max()) > 255 for t in tabs)
    body = b""
    for i, t in enumerate(tabs):
        zz = [int(v) for v in t[R.ZIGZAG]]
        body += bytes([0x10 | i]) + b"".join(struct.pack(">H", v) for v in zz) if wide else bytes([i]) + bytes(zz)
    out += R._segment(0xDB, body)
    comps = b"".join(bytes([i + 1, (s.hs << 4 | s.vs) if i == 0 and s.nc == 3 else 0x11, min(i, 1)]) for i in range(s.nc))
    out += R._segment(0xC1 if wide else 0xC0, struct.pack(">BHHB", 8, g.h, g.w, s.nc) + comps)
    if specs is None:
        specs = [R.DC_LUMA, R.AC_LUMA] + ([R.DC_CHROMA, R.AC_CHROMA] if s.nc == 3 else [])
    out += R._segment(0xC4, O.dht_body(specs))
    if g.dri:
        out += R._segment(0xDD, struct.pack(">H", g.dri))
    sel = b"".join(bytes([i + 1, 0x11 * min(i, 1)]) for i in range(s.nc))
    return out + R._segment(0xDA, bytes([s.nc]) + sel + b"\x00\x3f\x00")


def parts(src: Source, out: dict):
    """(coefficients, header, scan) of one output"""
    g = check(src, out)
    zz = gather(src, out, g)
    if out.get("optimize"):
        specs = O.tables(zz, g)
        return zz, headers(src, g, specs), O.scan(zz, g, specs)
    return zz, headers(src, g), R.scan(zz, g)


def transcode(data, outputs) -> list:
    """every output's file"""
    if not 1 <= len(outputs) <= MAX_OUTPUTS:
        raise Invalid("1 ... 16 outputs")
    src = data if isinstance(data, Source) else Source(data)
    files = []
    for o in outputs:
        _, head, scan = parts(src, o)
        files.append(head + scan + b"\xff\xd9")
    return files


# ---- the three uses, in pixels (vr180_convert_amd/jpeg_transcode_device.py) ---------------------------------------------------------------
def crop_output(src: Source, crop=None, **kw) -> dict:
    s = src.info
    x0, y0, w, h = (0, 0, s.w, s.h) if crop is None else crop
    if w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > s.w or y0 + h > s.h or x0 % src.mw or y0 % src.mh:
        raise ValueError("crop")
    return dict(width=w, height=h, regions=[(x0 // src.mw, y0 // src.mh, -(-w // src.mw), -(-h // src.mh), 0, 0)], **kw)


def split_outputs(src: Source, **kw) -> list:
    s = src.info
    if s.w % 2 or (s.w // 2) % src.mw:
        raise ValueError("half width")
    half = s.w // 2 // src.mw
    return [dict(width=s.w // 2, height=s.h, regions=[(x, 0, half, s.mcuy, 0, 0)], **kw) for x in (0, half)]


def swap_output(src: Source, **kw) -> dict:
    s = src.info
    if s.w % 2 or (s.w // 2) % src.mw:
        raise ValueError("half width")
    half = s.w // 2 // src.mw
    return dict(width=s.w, height=s.h, regions=[(half, 0, half, s.mcuy, 0, 0), (0, 0, half, s.mcuy, half, 0)], **kw)


def transcode_jpeg(data, *, crop=None, optimize=False, restart_mcus=None) -> bytes:
    src = Source(data)
    return transcode(src, [crop_output(src, crop, optimize=optimize, restart_mcus=restart_mcus)])[0]


def split_sbs_jpeg(data, *, optimize=False, restart_mcus=None):
    src = Source(data)
    return tuple(transcode(src, split_outputs(src, optimize=optimize, restart_mcus=restart_mcus)))


def swap_sbs_jpeg(data, *, optimize=False, restart_mcus=None) -> bytes:
    src = Source(data)
    return transcode(src, [swap_output(src, optimize=optimize, restart_mcus=restart_mcus)])[0]
