"""Lossless join, rotation and flip of JPEG files on the MI355X (``v1c_jpeg_compose``, csrc/kernels_jpegxf.hip): rectangles of MCUs of
up to four files are rotated, flipped or transposed in the DCT domain and placed into one output.  Each file is decoded by the device
decoder's entropy stage into a coefficient store of its own, one gather kernel moves the MCUs, the luma blocks within an MCU and the
coefficients within a block and flips the signs of the odd frequencies along a mirrored axis, and the device encoder's stages behind
its transform code the result: no inverse DCT, no pixels, no forward DCT, so no coefficient's magnitude changes and no JPEG generation
is lost.  What ``jpegtran -rotate / -flip / -transpose`` does, and a join of several files that it does not.

Files as ``transcode_jpeg`` takes them, all of one component count and sampling; a transposing transform (``transpose``, ``rot90``,
``rot270``, ``transverse``) not on 4:2:2 files.  The regions of one output must share their quantisation tables, transposed where a
region transposes.  ``NotImplementedError`` / ``CorruptJPEG`` / ``ValueError`` as ``transcode_regions``, all from host-only checks:
nothing falls back silently.  The sources' APPn and COM segments (EXIF, XMP, ICC) are not carried over.  INTEGRATION.md section 10
has the contract, ``tests/jpgxf_ref.py`` restates it.
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import Any, Sequence

from . import _native
from .jpeg_decode_device import _Last, _Report, _bytes_of, _check
from .jpeg_transcode_device import HEADER_XC_MAX, MAX_OUTPUTS, MAX_REGIONS, _output_fields, _restart, _run_outputs, probe_mcu

MAX_SOURCES = 4     # V1C_JPEG_XF_MAX_SOURCES

TRANSFORMS = {"none": 0, "flip_h": 1, "flip_v": 2, "rot180": 3, "transpose": 4, "rot90": 5, "rot270": 6, "transverse": 7}
_MIRROR_X, _MIRROR_Y, _TRANSPOSE = 1, 2, 4
# EXIF orientation (tag 0x0112) to the transform that makes the image upright
EXIF_TRANSFORMS = {1: "none", 2: "flip_h", 3: "rot180", 4: "flip_v", 5: "transpose", 6: "rot90", 7: "transverse", 8: "rot270"}


class XfSource(C.Structure):
    """``v1c_jpeg_xf_source`` (include/vr180_remap.h)"""
    _fields_ = [("file", C.c_char_p), ("size", C.c_uint64)]


class XfRegion(C.Structure):
    """``v1c_jpeg_xf_region`` (include/vr180_remap.h): in MCUs"""
    _fields_ = [(n, C.c_int32) for n in ("source", "transform", "src_x", "src_y", "nx", "ny", "dst_x", "dst_y")]


class XfOutput(C.Structure):
    """``v1c_jpeg_xf_output`` (include/vr180_remap.h)"""
    _fields_ = _output_fields(XfRegion)


_last = _Last()


def last_compose_report() -> dict:
    """what the calling thread's last composition did: per source the ``segments``, ``subsequences`` and ``rounds`` of its decode, and every output's
    scan ``sizes``"""
    return _last.get()


def transform_code(transform: Any) -> int:
    """the code of a transform given by name (``TRANSFORMS``), ``None`` for none"""
    if transform is None:
        return 0
    if not isinstance(transform, str) or transform not in TRANSFORMS:
        raise ValueError(f"a transform is one of {', '.join(TRANSFORMS)}, not {transform!r}")
    return TRANSFORMS[transform]


def compose_regions(sources: Sequence[Any], outputs: Sequence[dict], *, device: Any = None, subseq_bits: int = 0) -> list[bytes]:
    """The general call: ``sources`` are 1 ... 4 files (bytes or paths); every output is ``{"width", "height", "regions": [(source,
    transform, src_x, src_y, nx, ny, dst_x, dst_y), ...]}`` with the regions in MCUs and the transform a name, and optionally
    ``"restart_mcus"`` (None: one MCU row; 0: none) and ``"optimize"``.  A region is placed as ``ny x nx`` MCUs where it transposes.
    Returns every output's file.  All checks that need no device are made before one is touched."""
    datas = [_bytes_of(s) for s in sources]
    lib = _native.lib()
    ns, n = len(datas), len(outputs)
    if not 1 <= ns <= MAX_SOURCES:
        raise ValueError(f"1 ... {MAX_SOURCES} sources, not {ns}")
    if not 1 <= n <= MAX_OUTPUTS:
        raise ValueError(f"1 ... {MAX_OUTPUTS} outputs, not {n}")
    _, _, mw, _ = probe_mcu(datas[0])
    srcs = (XfSource * ns)(*[XfSource(d, len(d)) for d in datas])
    outs = (XfOutput * n)()
    keep, first = [], []
    for o, spec in zip(outs, outputs):
        regs = [tuple(r) for r in spec["regions"]]
        if not 1 <= len(regs) <= MAX_REGIONS or any(len(r) != 8 for r in regs):
            raise ValueError(f"an output has 1 ... {MAX_REGIONS} regions of (source, transform, src_x, src_y, nx, ny, dst_x, dst_y)")
        regs = [(int(r[0]), transform_code(r[1])) + tuple(int(v) for v in r[2:]) for r in regs]
        arr = (XfRegion * len(regs))(*[XfRegion(*r) for r in regs])
        keep.append(arr)
        first.append(regs[0])
        o.width, o.height = int(spec["width"]), int(spec["height"])
        o.restart_mcus = _restart(spec.get("restart_mcus"), o.width, mw)
        o.optimize, o.nregions, o.regions = int(bool(spec.get("optimize", False))), len(regs), arr
    _check(lib.v1c_jpeg_compose_check(ns, srcs, n, outs, None), "v1c_jpeg_compose")
    reps = (_Report * ns)()

    def header(i: int, o: XfOutput, head: Any) -> int:
        source, code = first[i][:2]  # (region 0's file and transform: whose tables the output has)
        d = datas[source]
        return lib.v1c_jpeg_header_xf(d, len(d), o.width, o.height, o.restart_mcus, int(bool(code & _TRANSPOSE)), o.dht if o.optimize else None,
                                      o.dht_size, head, HEADER_XC_MAX)

    files = _run_outputs(
        outs, device, lambda o: lib.v1c_jpeg_compose_bound(datas[0], len(datas[0]), o.width, o.height, o.restart_mcus),
        lambda index, stream: _check(lib.v1c_jpeg_compose(index, stream, ns, srcs, n, outs, int(subseq_bits), reps), "v1c_jpeg_compose"),
        header, "v1c_jpeg_header_xf")
    _last.clear()
    _last.update(sources=[dict(segments=r.segments, subsequences=r.subsequences, rounds=r.rounds) for r in reps], sizes=[int(o.size) for o in outs])
    return files


def _transformed(h: int, w: int, mw: int, mh: int, code: int, trim: bool) -> tuple[int, int, int, int]:
    """(width, height, nx, ny): the pixel size of the whole image under the transform and the source MCUs it takes.  A mirrored axis
    that is no multiple of the MCU is refused, or with ``trim`` loses its partial last column or row first."""
    mirrored_w = bool(code & (_MIRROR_Y if code & _TRANSPOSE else _MIRROR_X))  # (a mirror behind the transpose mirrors the source's other axis)
    mirrored_h = bool(code & (_MIRROR_X if code & _TRANSPOSE else _MIRROR_Y))
    for axis, size, m, mirrored in (("width", w, mw, mirrored_w), ("height", h, mh, mirrored_h)):
        if mirrored and size % m and (not trim or size < m):
            raise ValueError(f"the {axis} {size} is no multiple of the file's {m}-pixel MCU, and the transform mirrors it: a lossless mirror "
                             f"needs whole MCUs" + ("" if trim else " (trim=True cuts the partial one off)"))
    if mirrored_w:
        w -= w % mw
    if mirrored_h:
        h -= h % mh
    nx, ny = -(-w // mw), -(-h // mh)
    return (h, w, nx, ny) if code & _TRANSPOSE else (w, h, nx, ny)


def transform_jpeg(data_or_path: Any, op: str, *, trim: bool = False, optimize: bool = False, restart_mcus: int | None = None,
                   device: Any = None) -> bytes:
    """The whole image flipped, rotated or transposed without a JPEG generation; ``op`` is one of ``TRANSFORMS``.  A mirrored axis whose
    size is no multiple of the MCU raises ``ValueError`` (jpegtran's ``-perfect``); with ``trim=True`` its partial last MCU column or
    row is cut off first (jpegtran's ``-trim``)."""
    data = _bytes_of(data_or_path)
    code = transform_code(op)
    h, w, mw, mh = probe_mcu(data)
    ow, oh, nx, ny = _transformed(h, w, mw, mh, code, trim)
    return compose_regions([data], [dict(width=ow, height=oh, optimize=optimize, restart_mcus=restart_mcus, regions=[(0, op, 0, 0, nx, ny, 0, 0)])],
                           device=device)[0]


def join_sbs_jpeg(left: Any, right: Any, *, left_transform: str | None = None, right_transform: str | None = None, trim: bool = False,
                  optimize: bool = False, restart_mcus: int | None = None, device: Any = None) -> bytes:
    """One side-by-side file of two files, each eye transformed on the way: the inverse of ``split_sbs_jpeg``.  ``ValueError`` unless
    both eyes end up the same height and the left eye's width is a multiple of the MCU width (``trim=True`` cuts it)."""
    l, r = _bytes_of(left), _bytes_of(right)
    lc, rc = transform_code(left_transform), transform_code(right_transform)
    lh, lw, mw, mh = probe_mcu(l)
    rh, rw, rmw, rmh = probe_mcu(r)
    low, loh, lnx, lny = _transformed(lh, lw, mw, mh, lc, trim)
    row, roh, rnx, rny = _transformed(rh, rw, rmw, rmh, rc, trim)
    m = mh if lc & _TRANSPOSE else mw  # the MCU width of the left eye as it is placed
    if low % m:
        if not trim or low < m:
            raise ValueError(f"the left eye's width {low} is no multiple of the {m}-pixel MCU: the right eye cannot start on the MCU grid"
                             + ("" if trim else " (trim=True cuts the partial column off)"))
        low -= low % m
        if lc & _TRANSPOSE:
            lny = low // m
        else:
            lnx = low // m
    if loh != roh:
        raise ValueError(f"the eyes end up {loh} and {roh} pixels high: a side-by-side file needs one height")
    placed = lny if lc & _TRANSPOSE else lnx
    out = dict(width=low + row, height=loh, optimize=optimize, restart_mcus=restart_mcus,
               regions=[(0, left_transform or "none", 0, 0, lnx, lny, 0, 0), (1, right_transform or "none", 0, 0, rnx, rny, placed, 0)])
    return compose_regions([l, r], [out], device=device)[0]


def sbs_from_vr180_photo(data_or_path: Any, **kw: Any) -> bytes:
    """The side-by-side file of a Google VR180 photo (``read_vr180_photo``, then ``join_sbs_jpeg`` with ``kw``)."""
    from .vr180_photo import read_vr180_photo

    left, right, _ = read_vr180_photo(_bytes_of(data_or_path))
    return join_sbs_jpeg(left, right, **kw)


def exif_orientation(data: bytes) -> int:
    """EXIF tag 0x0112 of the file's first APP1 "Exif" segment, in either byte order; 1 where there is none or it is outside 1 ... 8"""
    data = bytes(data)
    at = 2
    while at + 4 <= len(data) and data[at] == 0xFF:
        marker, size = data[at + 1], struct.unpack(">H", data[at + 2:at + 4])[0]
        if marker == 0xDA or size < 2:
            break
        body = data[at + 4:at + 2 + size]
        at += 2 + size
        if marker != 0xE1 or body[:6] != b"Exif\x00\x00":
            continue
        tiff = body[6:]
        if len(tiff) < 8 or tiff[:2] not in (b"II", b"MM"):
            return 1
        e = "<" if tiff[:2] == b"II" else ">"
        if struct.unpack(e + "H", tiff[2:4])[0] != 42:
            return 1
        ifd = struct.unpack(e + "I", tiff[4:8])[0]
        if ifd + 2 > len(tiff):
            return 1
        count = struct.unpack(e + "H", tiff[ifd:ifd + 2])[0]
        for i in range(count):
            entry = tiff[ifd + 2 + 12 * i:ifd + 14 + 12 * i]
            if len(entry) < 12:
                return 1
            tag, kind, n = struct.unpack(e + "HHI", entry[:8])
            if tag == 0x0112:
                value = struct.unpack(e + "H", entry[8:10])[0] if kind == 3 and n == 1 else 1
                return value if 1 <= value <= 8 else 1
        return 1
    return 1


def normalize_orientation_jpeg(data_or_path: Any, *, trim: bool = False, optimize: bool = False, restart_mcus: int | None = None,
                               device: Any = None) -> bytes:
    """The file with its EXIF orientation baked in: the transform of ``EXIF_TRANSFORMS`` applied losslessly.  The output carries no
    EXIF, as every transcoder output, so it is upright by definition; orientation 1 or no tag: the image coded again as it is."""
    data = _bytes_of(data_or_path)
    return transform_jpeg(data, EXIF_TRANSFORMS[exif_orientation(data)], trim=trim, optimize=optimize, restart_mcus=restart_mcus, device=device)


__all__ = ["compose_regions", "transform_jpeg", "join_sbs_jpeg", "sbs_from_vr180_photo", "normalize_orientation_jpeg", "exif_orientation",
           "last_compose_report", "transform_code", "TRANSFORMS", "EXIF_TRANSFORMS"]
