"""Lossless crop, split and swap of JPEG files on the MI355X (``v1c_jpeg_transcode``, csrc/kernels_jpegxc.hip): the file is cut on MCU
boundaries in the DCT domain.  The device decoder's entropy stage leaves the file's quantised coefficients in its store, a gather kernel
copies rectangles of MCUs into the device encoder's store, and the encoder's stages behind its transform code them again: no inverse
DCT, no pixels, no forward DCT, so no coefficient changes and no JPEG generation is lost.  Only the file's bytes go to the device and
only the finished scans come back; the header segments -- the FILE's quantisation tables and sampling factors -- are put around them
here (``v1c_jpeg_header_xc``).

Files of one component, or of three in 4:4:4, 4:2:2 or 4:2:0, baseline or extended sequential, with any tables and any restart
interval; an MCU is 8 x 8 pixels, 16 x 8 in 4:2:2, 16 x 16 in 4:2:0.  Progressive files and whatever else ``decode_jpeg_tensor`` refuses raise
``NotImplementedError`` from a host-only parse, a damaged file ``CorruptJPEG``, a cut off the MCU grid ``ValueError``: nothing falls
back silently.  The source's APPn and COM segments (EXIF, XMP, ICC) are not carried over.  INTEGRATION.md section 9 has the
contract, ``tests/jpgxc_ref.py`` restates it.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Sequence

from . import _native
from .jpeg_decode_device import _Info, _Last, _Report, _bytes_of, _check
from .jpeg_device import DHT_MAX

MAX_REGIONS = 16    # V1C_JPEG_XC_MAX_REGIONS
MAX_OUTPUTS = 16    # V1C_JPEG_XC_MAX_OUTPUTS
HEADER_XC_MAX = 2048  # V1C_JPEG_HEADER_XC_MAX


class XcRegion(C.Structure):
    """``v1c_jpeg_xc_region`` (include/vr180_remap.h): in MCUs"""
    _fields_ = [(n, C.c_int32) for n in ("src_x", "src_y", "nx", "ny", "dst_x", "dst_y")]


def _output_fields(region: type) -> list:
    """the fields of ``v1c_jpeg_xc_output`` and ``v1c_jpeg_xf_output`` (include/vr180_remap.h), which differ in their regions' type"""
    return [("width", C.c_int32), ("height", C.c_int32), ("restart_mcus", C.c_int32), ("optimize", C.c_int32), ("nregions", C.c_int32),
            ("reserved", C.c_int32), ("regions", C.POINTER(region)), ("out_host", C.c_void_p), ("capacity", C.c_uint64),
            ("size", C.c_uint64), ("dht_size", C.c_uint32), ("dht", C.c_uint8 * DHT_MAX)]


class XcOutput(C.Structure):
    """``v1c_jpeg_xc_output`` (include/vr180_remap.h)"""
    _fields_ = _output_fields(XcRegion)


_last = _Last()


def last_transcode_report() -> dict:
    """what the calling thread's last transcode did: ``segments``, ``subsequences`` and ``rounds`` of the decode, and every output's scan ``sizes``"""
    return _last.get()


def probe_mcu(data_or_path: Any) -> tuple[int, int, int, int]:
    """(height, width, MCU width, MCU height) of a file by the host-only parse; ``NotImplementedError`` / ``CorruptJPEG`` as
    ``decode_jpeg_tensor``."""
    data = _bytes_of(data_or_path)
    info = _Info()
    _check(_native.lib().v1c_jpeg_decode_info(data, len(data), C.byref(info)), "v1c_jpeg_decode_info")
    colour = info.components == 3
    return info.height, info.width, 8 * (info.h_samp if colour else 1), 8 * (info.v_samp if colour else 1)


def _restart(restart_mcus: Any, width: int, mw: int) -> int:
    """MCUs per restart interval of an output: ``None`` -- one MCU row, as ``encode_jpeg_tensor`` chooses --, 0 for none, or 1 ... 65535"""
    r = min(65535, -(-width // mw)) if restart_mcus is None else int(restart_mcus)
    if not 0 <= r <= 65535:
        raise ValueError("restart_mcus must be 0 (no restart markers) ... 65535, or None for one MCU row")
    return r


def _run_outputs(outs: Any, device: Any, bound: Any, call: Any, header: Any, header_name: str) -> list[bytes]:
    """What ``transcode_regions`` and ``compose_regions`` do behind their host-only checks, the device only from here on: one host
    buffer carved into every output's ``out_host`` by ``bound(o)``, the entry by ``call(device index, stream)``, and every output's
    file -- the header that ``header(i, o, head)`` writes into the ``HEADER_XC_MAX`` bytes of ``head`` (returning their number, or the
    code of ``header_name``), its scan and EOI."""
    from .jpeg_device import _host_buffer
    from .remapper import _device, _stream_ptr

    dev = _device(device)
    bounds = [int(bound(o)) for o in outs]
    buf = _host_buffer(dev, sum(bounds))
    at = 0
    for o, b in zip(outs, bounds):
        o.out_host, o.capacity = buf.data_ptr() + at, b
        at += b
    call(dev.index, _stream_ptr(dev))
    host, at, files = buf.numpy(), 0, []
    for i, (o, b) in enumerate(zip(outs, bounds)):
        head = (C.c_uint8 * HEADER_XC_MAX)()
        m = header(i, o, head)
        if m < 0:
            _check(int(m), header_name)
        files.append(bytes(head[:m]) + host[at:at + int(o.size)].tobytes() + b"\xff\xd9")
        at += b
    return files


def transcode_regions(data_or_path: Any, outputs: Sequence[dict], *, device: Any = None) -> list[bytes]:
    """The general call: every output is ``{"width", "height", "regions": [(src_x, src_y, nx, ny, dst_x, dst_y), ...]}`` with the regions
    in MCUs, and optionally ``"restart_mcus"`` (None: one MCU row; 0: none) and ``"optimize"``.  Returns every output's file.  All
    checks that need no device are made before one is touched."""
    data = _bytes_of(data_or_path)
    lib = _native.lib()
    n = len(outputs)
    if not 1 <= n <= MAX_OUTPUTS:
        raise ValueError(f"1 ... {MAX_OUTPUTS} outputs, not {n}")
    _, _, mw, _ = probe_mcu(data)
    outs = (XcOutput * n)()
    keep = []
    for o, spec in zip(outs, outputs):
        regs = [tuple(int(v) for v in r) for r in spec["regions"]]
        if not 1 <= len(regs) <= MAX_REGIONS or any(len(r) != 6 for r in regs):
            raise ValueError(f"an output has 1 ... {MAX_REGIONS} regions of (src_x, src_y, nx, ny, dst_x, dst_y)")
        arr = (XcRegion * len(regs))(*[XcRegion(*r) for r in regs])
        keep.append(arr)
        o.width, o.height = int(spec["width"]), int(spec["height"])
        o.restart_mcus = _restart(spec.get("restart_mcus"), o.width, mw)
        o.optimize, o.nregions, o.regions = int(bool(spec.get("optimize", False))), len(regs), arr
    _check(lib.v1c_jpeg_transcode_check(data, len(data), n, outs, None), "v1c_jpeg_transcode")
    rep = _Report()
    files = _run_outputs(
        outs, device, lambda o: lib.v1c_jpeg_transcode_bound(data, len(data), o.width, o.height, o.restart_mcus),
        lambda index, stream: _check(lib.v1c_jpeg_transcode(index, stream, data, len(data), n, outs, 0, C.byref(rep)), "v1c_jpeg_transcode"),
        lambda i, o, head: lib.v1c_jpeg_header_xc(data, len(data), o.width, o.height, o.restart_mcus, o.dht if o.optimize else None,
                                                  o.dht_size, head, HEADER_XC_MAX), "v1c_jpeg_header_xc")
    _last.clear()
    _last.update(segments=rep.segments, subsequences=rep.subsequences, rounds=rep.rounds, sizes=[int(o.size) for o in outs])
    return files


def _crop_output(h: int, w: int, mw: int, mh: int, crop: Any, kw: dict) -> dict:
    x0, y0, cw, ch = (0, 0, w, h) if crop is None else (int(v) for v in crop)
    if cw < 1 or ch < 1 or x0 < 0 or y0 < 0 or x0 + cw > w or y0 + ch > h:
        raise ValueError(f"crop {(x0, y0, cw, ch)} leaves the {w} x {h} image")
    if x0 % mw or y0 % mh:
        raise ValueError(f"the crop's origin ({x0}, {y0}) is no multiple of the file's {mw} x {mh} MCU: a lossless cut lies on the MCU grid")
    return dict(width=cw, height=ch, regions=[(x0 // mw, y0 // mh, -(-cw // mw), -(-ch // mh), 0, 0)], **kw)


def _half_mcus(w: int, mw: int) -> int:
    if w % 2 or (w // 2) % mw:
        raise ValueError(f"a side-by-side file is cut losslessly where its width is even and half of it a multiple of the MCU width: "
                         f"{w} and {mw} are not")
    return w // 2 // mw


def transcode_jpeg(data_or_path: Any, *, crop: tuple[int, int, int, int] | None = None, optimize: bool = False,
                   restart_mcus: int | None = None, device: Any = None) -> bytes:
    """The file cut to ``crop = (x0, y0, w, h)`` in pixels without a JPEG generation: every sample a reader decodes from the kept MCUs
    is the sample it decodes from the source.  ``x0`` and ``y0`` must be multiples of the MCU (``ValueError``); ``w`` and ``h`` are free:
    the last MCU column and row are kept whole and the size says how much of them shows, as in the source.  ``crop=None``: the whole
    image, coded again.  ``optimize``: Huffman tables built for the output on the device; ``restart_mcus``: MCUs per restart interval
    of the output (None: one MCU row, as ``encode_jpeg_tensor``; 0: none)."""
    data = _bytes_of(data_or_path)
    h, w, mw, mh = probe_mcu(data)
    return transcode_regions(data, [_crop_output(h, w, mw, mh, crop, dict(optimize=optimize, restart_mcus=restart_mcus))], device=device)[0]


def split_sbs_jpeg(data_or_path: Any, *, optimize: bool = False, restart_mcus: int | None = None, device: Any = None) -> tuple[bytes, bytes]:
    """The left and the right half of a side-by-side file as two files, in one call.  ``ValueError`` unless the width is even and half
    of it a multiple of the MCU width."""
    data = _bytes_of(data_or_path)
    h, w, mw, mh = probe_mcu(data)
    half, rows = _half_mcus(w, mw), -(-h // mh)
    kw = dict(width=w // 2, height=h, optimize=optimize, restart_mcus=restart_mcus)
    left, right = transcode_regions(data, [dict(regions=[(0, 0, half, rows, 0, 0)], **kw), dict(regions=[(half, 0, half, rows, 0, 0)], **kw)],
                                    device=device)
    return left, right


def swap_sbs_jpeg(data_or_path: Any, *, optimize: bool = False, restart_mcus: int | None = None, device: Any = None) -> bytes:
    """A side-by-side file with its halves exchanged.  ``ValueError`` unless the width is even and half of it a multiple of the MCU
    width."""
    data = _bytes_of(data_or_path)
    h, w, mw, mh = probe_mcu(data)
    half, rows = _half_mcus(w, mw), -(-h // mh)
    return transcode_regions(data, [dict(width=w, height=h, optimize=optimize, restart_mcus=restart_mcus,
                                         regions=[(half, 0, half, rows, 0, 0), (0, 0, half, rows, half, 0)])], device=device)[0]


__all__ = ["transcode_jpeg", "split_sbs_jpeg", "swap_sbs_jpeg", "transcode_regions", "last_transcode_report", "probe_mcu"]
