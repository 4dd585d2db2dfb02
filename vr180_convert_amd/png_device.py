"""PNG files of device-resident results, deflated on the MI355X (``v1c_png_deflate``, csrc/kernels_png.hip): the image is filtered,
run-length tokenised, Huffman-coded and bit-packed by HIP kernels, only the compressed stream comes to the host, and
``_png.assemble`` wraps it into a standard PNG that every reader decodes (and, with the Up filter, ``_png.decode`` in parallel).

Not zlib level 1: deflate restricted to literals and distance-1 matches, one dynamic Huffman block per band.  The files are larger
than the host writer's (INTEGRATION.md section 6 has the contract and the measured sizes); ``tests/png_ref.py`` restates the stream.
"""
from __future__ import annotations

import ctypes as C
import threading
from pathlib import Path
from typing import Any

import numpy as np
import torch

from . import _abi, _native, _png
from .remapper import _stream_ptr

FILTERS = {"up": 2, "paeth": 4}
BAND_BYTES = 192 * 1024  # scanline bytes a default band aims at: an 8192 x 4096 side-by-side frame gets 8-row bands, 512 of them


class Band(C.Structure):
    _fields_ = [("row0", C.c_uint32), ("row1", C.c_uint32), ("offset", C.c_uint64), ("size", C.c_uint64), ("adler32", C.c_uint32),
                ("stored", C.c_uint32)]


def default_band_rows(height: int, stride: int) -> int:
    """rows per band when the caller names none: about BAND_BYTES of scanlines, so that large images fill the device"""
    return max(1, min(height, -(-BAND_BYTES // stride)))


# Per calling thread, .pinned: {device index: the page-locked buffer the thread's streams land in}, grown on demand and kept until the
# thread ends.  The engine call releases the GIL and the callers read views of the buffer after it, so a buffer shared between threads
# would hand one thread another's stream.
_TLS = threading.local()


def _host_buffer(dev: torch.device, nbytes: int) -> torch.Tensor:
    pinned = _TLS.__dict__.setdefault("pinned", {})
    buf = pinned.get(dev.index)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, pin_memory=True)
        pinned[dev.index] = buf
    return buf


def _image(t: torch.Tensor) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("the device PNG encoder takes CUDA tensors")
    if t.dtype not in (torch.uint8, torch.uint16):
        raise TypeError(f"the device PNG encoder takes uint8 / uint16 tensors, not {t.dtype}")
    if t.dim() == 2:
        t = t[..., None]
    if t.dim() != 3 or t.shape[2] not in (1, 3, 4) or t.shape[0] == 0 or t.shape[1] == 0:
        raise ValueError(f"the device PNG encoder takes non-empty (H, W[, C]) images with C 1, 3 or 4, not {tuple(t.shape)}")
    # rows may be pitched (one half of a side-by-side tensor); pixels and channels must be dense
    if (t.shape[2] > 1 and t.stride(2) != 1) or (t.shape[1] > 1 and t.stride(1) != t.shape[2]) or (t.shape[0] > 1 and t.stride(0) < t.shape[1] * t.shape[2]):
        t = t.contiguous()
    return t


def deflate_tensor(t: torch.Tensor, *, filter: str = "up", band_rows: int | None = None):
    """``(segments, bands)`` of a device image on the current stream: a uint8 view of the band segments (valid until the next call
    on this device from this thread: the buffer behind it belongs to the calling thread) and one ``(row0, row1, offset, size, adler32,
    stored)`` tuple per band."""
    if filter not in FILTERS:
        raise ValueError(f"filter must be one of {sorted(FILTERS)}, not {filter!r}")
    t = _image(t)
    h, w, cn = (int(v) for v in t.shape)
    nb = t.element_size()
    rows = default_band_rows(h, 1 + w * cn * nb) if band_rows is None else int(band_rows)
    if rows < 1:
        raise ValueError("band_rows must be at least 1")
    lib = _native.lib()
    depth = _abi.DEPTH_16U if nb == 2 else _abi.DEPTH_8U
    cap = int(lib.v1c_png_bound(h, w, cn, depth, rows))
    if cap == 0:
        raise ValueError(f"image {w} x {h} x {cn} with {rows}-row bands is outside what v1c_png_deflate takes")
    dev = t.device
    buf = _host_buffer(dev, cap)
    n_bands = -(-h // min(rows, h))
    bands = (Band * n_bands)()
    count, size = C.c_int32(0), C.c_uint64(0)
    pitch = t.stride(0) * nb if h > 1 else w * cn * nb
    rc = lib.v1c_png_deflate(dev.index, _stream_ptr(dev), t.data_ptr(), h, w, pitch, cn, depth, FILTERS[filter], rows, buf.data_ptr(),
                             buf.numel(), bands, C.byref(count), C.byref(size))
    _native.check(rc, "v1c_png_deflate")
    out = [(b.row0, b.row1, b.offset, b.size, b.adler32, b.stored) for b in bands[:count.value]]
    return buf.numpy()[:size.value], out


def _parts(t: torch.Tensor, filter: str, band_rows: int | None, threads: int | None) -> list:
    segments, bands = deflate_tensor(t, filter=filter, band_rows=band_rows)
    shape = tuple(t.shape) + (1,) * (3 - t.dim())
    return _png.assemble_parts(segments, [b[:5] for b in bands], width=int(shape[1]), height=int(shape[0]), channels=int(shape[2]),
                               bit_depth=8 * t.element_size(), filter_type=FILTERS[filter], threads=threads)


def encode_png_tensor(t: torch.Tensor, *, filter: str = "up", band_rows: int | None = None, threads: int | None = None) -> bytes:
    """PNG bytes of a CUDA ``uint8`` / ``uint16`` tensor ``(H, W[, C])`` in cv2 channel order (C 1, 3 or 4), deflated on the device
    on the current stream.  ``filter``: ``"up"`` (``_png.decode`` reads the file in parallel) or ``"paeth"`` (smaller on drawn
    content; general readers only).  ``threads``: of the IDAT chunk's CRC-32 on the host.  Two calls give identical bytes."""
    return b"".join(_parts(t, filter, band_rows, threads))


def imwrite_tensor(path: Any, t: torch.Tensor, *, filter: str = "up", band_rows: int | None = None, threads: int | None = None) -> None:
    """``encode_png_tensor`` into a file (the stream goes from the page-locked buffer to the file without a copy in between)"""
    with open(path, "wb") as f:
        for part in _parts(t, filter, band_rows, threads):
            f.write(part)


def eligible(path: Any, result: Any) -> bool:
    """whether ``device_png=True`` writes this result through the device encoder: a ``.png`` path and a uint8 / uint16 device tensor"""
    return (isinstance(path, (str, Path)) and Path(path).suffix.lower() == ".png" and isinstance(result, torch.Tensor) and result.is_cuda
            and result.dtype in (torch.uint8, torch.uint16))


__all__ = ["encode_png_tensor", "imwrite_tensor", "deflate_tensor", "default_band_rows", "eligible"]
