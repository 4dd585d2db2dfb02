"""JPEG files of device-resident results, encoded on the MI355X (``v1c_jpeg_encode``, csrc/kernels_jpeg.hip): colour conversion,
chroma downsampling, the forward DCT, quantisation, Huffman coding, byte stuffing and the restart markers are HIP kernels, only the
finished scan comes to the host, and the header segments (``v1c_jpeg_header``) and EOI are put around it here.

Baseline sequential JPEG with the standard tables, which every reader decodes -- not libjpeg's output byte for byte: the chroma
rounding differs and the file carries restart markers (INTEGRATION.md section 7 has the contract and the measured sizes;
``tests/jpg_ref.py`` restates the file).
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Any

import torch

from . import _native
from .remapper import _stream_ptr

SUBSAMPLINGS = {"444": 0, "420": 2}  # V1C_JPEG_444 / V1C_JPEG_420
HEADER_MAX = 1024                    # V1C_JPEG_HEADER_MAX


def default_restart_mcus(height: int, width: int, channels: int, subsampling: str = "420") -> int:
    """MCUs per restart interval when the caller names none: one MCU row, so that the intervals follow the image's rows (a decoder
    can start at any of them) and an 8192 x 4096 frame has 256 (4:2:0) or 512 (4:4:4) of them.  The kernels' work does not depend
    on it: every lane's work is bounded whatever the interval."""
    m = 16 if (channels != 1 and subsampling == "420") else 8
    return min(65535, -(-width // m))


_pinned: dict[int, torch.Tensor] = {}  # per device: the page-locked buffer the scan lands in, grown on demand


def _host_buffer(dev: torch.device, nbytes: int) -> torch.Tensor:
    buf = _pinned.get(dev.index)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, pin_memory=True)
        _pinned[dev.index] = buf
    return buf


def _image(t: torch.Tensor) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("the device JPEG encoder takes CUDA tensors")
    if t.dtype != torch.uint8:
        raise TypeError(f"the device JPEG encoder takes uint8 tensors, not {t.dtype}")
    if t.dim() == 2:
        t = t[..., None]
    if t.dim() != 3 or t.shape[2] not in (1, 3, 4) or t.shape[0] == 0 or t.shape[1] == 0:
        raise ValueError(f"the device JPEG encoder takes non-empty (H, W[, C]) images with C 1, 3 or 4, not {tuple(t.shape)}")
    # rows may be pitched (one half of a side-by-side tensor); pixels and channels must be dense
    if (t.shape[2] > 1 and t.stride(2) != 1) or (t.shape[1] > 1 and t.stride(1) != t.shape[2]) or (t.shape[0] > 1 and t.stride(0) < t.shape[1] * t.shape[2]):
        t = t.contiguous()
    return t


def _parts(t: torch.Tensor, quality: int, subsampling: str, restart_mcus: int | None) -> list:
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"subsampling must be one of {sorted(SUBSAMPLINGS)}, not {subsampling!r}")
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError("quality must be 1 ... 100")
    t = _image(t)
    h, w, cn = (int(v) for v in t.shape)
    if h > 65535 or w > 65535:
        raise ValueError(f"a baseline JPEG holds at most 65535 x 65535 pixels, not {w} x {h}")
    restart = default_restart_mcus(h, w, cn, subsampling) if restart_mcus is None else int(restart_mcus)
    if not 1 <= restart <= 65535:
        raise ValueError("restart_mcus must be 1 ... 65535")
    lib = _native.lib()
    sub = SUBSAMPLINGS[subsampling]
    head = (C.c_uint8 * HEADER_MAX)()
    n = lib.v1c_jpeg_header(h, w, cn, quality, sub, restart, head, HEADER_MAX)
    if n < 0:
        _native.check(int(n), "v1c_jpeg_header")
    cap = int(lib.v1c_jpeg_bound(h, w, cn, sub, restart))
    dev = t.device
    buf = _host_buffer(dev, cap)
    size = C.c_uint64(0)
    pitch = t.stride(0) if h > 1 else w * cn
    rc = lib.v1c_jpeg_encode(dev.index, _stream_ptr(dev), t.data_ptr(), h, w, pitch, cn, quality, sub, restart, buf.data_ptr(), buf.numel(),
                             C.byref(size))
    _native.check(rc, "v1c_jpeg_encode")
    return [bytes(head[:n]), buf.numpy()[:size.value], b"\xff\xd9"]


def encode_jpeg_tensor(t: torch.Tensor, *, quality: int = 95, subsampling: str = "420", restart_mcus: int | None = None) -> bytes:
    """JPEG bytes of a CUDA ``uint8`` tensor ``(H, W[, C])`` in cv2 channel order (C 1: greyscale, 3: YCbCr, 4: alpha dropped), encoded
    on the device on the current stream.  ``quality``: 1 ... 100, the IJG rule (95: the host writer's).  ``subsampling``: ``"420"``
    (cv2's and Pillow's at that quality) or ``"444"``.  ``restart_mcus``: MCUs per restart interval, 1 ... 65535
    (``default_restart_mcus``: one MCU row).  Two calls give identical bytes."""
    return b"".join(bytes(p) for p in _parts(t, quality, subsampling, restart_mcus))


def imwrite_jpeg_tensor(path: Any, t: torch.Tensor, *, quality: int = 95, subsampling: str = "420", restart_mcus: int | None = None) -> None:
    """``encode_jpeg_tensor`` into a file (the scan goes from the page-locked buffer to the file without a copy in between)"""
    with open(path, "wb") as f:
        for part in _parts(t, quality, subsampling, restart_mcus):
            f.write(part)


def eligible(path: Any, result: Any) -> bool:
    """whether ``device_jpeg=True`` writes this result through the device encoder: a ``.jpg`` / ``.jpeg`` path and a uint8 device tensor"""
    return (isinstance(path, (str, Path)) and Path(path).suffix.lower() in (".jpg", ".jpeg") and isinstance(result, torch.Tensor)
            and result.is_cuda and result.dtype == torch.uint8)


__all__ = ["encode_jpeg_tensor", "imwrite_jpeg_tensor", "default_restart_mcus", "eligible"]
