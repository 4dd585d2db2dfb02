"""JPEG files decoded on the MI355X into device tensors (``v1c_jpeg_decode``, csrc/kernels_jpegdec.hip): only the file's bytes cross
PCIe.  The host parses the markers and walks the scan's 0xFF bytes; unstuffing, Huffman decoding -- parallel over subsequences of
the scan whose entry states are found by iteration --, the DC scan, dequantisation, the inverse DCT, chroma upsampling and colour
conversion are HIP kernels.

Baseline and extended sequential Huffman files (SOF0 / SOF1, 8-bit) of one component or of three in 4:4:4, 4:2:2 or 4:2:0, with any
tables and any restart interval or none; the pixels are libjpeg's default decode (INTEGRATION.md section 8 has the contract,
``tests/jpgdec_ref.py`` restates it).  Anything else raises ``NotImplementedError`` from a host-only parse, a damaged file
``ValueError``: nothing falls back silently.
"""
from __future__ import annotations

import ctypes as C
import logging
from pathlib import Path
from typing import Any

import torch

from . import _abi, _native
from .remapper import _device, _stream_ptr


class _Info(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("height", "width", "components", "h_samp", "v_samp", "restart_interval")]


class _Report(C.Structure):
    _fields_ = [("segments", C.c_uint32), ("subsequences", C.c_uint32), ("rounds", C.c_uint32), ("reserved", C.c_uint32),
                ("error_pos", C.c_uint64)]


LOG = logging.getLogger(__name__)
_last: dict = {}


class CorruptJPEG(ValueError):
    """the file is damaged (``V1C_E_CORRUPT``): by the host parse, or by the last pass of the decode on the device"""


def _check(rc: int, what: str) -> None:
    if rc == _abi.E_CORRUPT:
        raise CorruptJPEG(f"{what}: {_native.lib().v1c_last_error().decode('utf-8', 'replace')}")
    _native.check(rc, what)


def _bytes_of(data_or_path: Any) -> bytes:
    if isinstance(data_or_path, (str, Path)):
        return Path(data_or_path).read_bytes()
    return bytes(data_or_path)


def probe(data_or_path: Any) -> tuple[int, int, int]:
    """(height, width, components) of a file the device decodes, by the host-only parse; ``NotImplementedError`` / ``ValueError`` as
    ``decode_jpeg_tensor``"""
    data = _bytes_of(data_or_path)
    info = _Info()
    _check(_native.lib().v1c_jpeg_decode_info(data, len(data), C.byref(info)), "v1c_jpeg_decode_info")
    return info.height, info.width, info.components


def decode_jpeg_tensor(data_or_path: Any, *, device: Any = None, channels: int = 3, subseq_bits: int | None = None) -> torch.Tensor:
    """A JPEG file (its bytes, or a path) as a CUDA ``uint8`` tensor in cv2 channel order, decoded on the device on the current
    stream: ``(H, W, 3)`` BGR (a grey file replicated, as ``cv2.imread`` does), or ``(H, W)`` with ``channels=1`` for a grey file.
    ``subseq_bits``: bits of the scan one lane decodes, a multiple of 32 from 256 (None: the engine's default); the pixels do not
    depend on it.  EXIF orientation is not applied.  Raises ``NotImplementedError`` for a file outside the device decoder's scope and
    ``CorruptJPEG`` (a ``ValueError``) for a damaged one; ``last_decode_report()`` tells what the call did."""
    if channels not in (1, 3):
        raise ValueError("channels must be 1 or 3")
    S = 0 if subseq_bits is None else int(subseq_bits)
    if S and (S % 32 or S < 256):
        raise ValueError("subseq_bits must be a multiple of 32, at least 256")
    data = _bytes_of(data_or_path)
    h, w, nc = probe(data)
    if channels == 1 and nc != 1:
        raise ValueError("channels=1 takes a grey file")
    dev = _device(device)
    out = torch.empty((h, w) if channels == 1 else (h, w, 3), dtype=torch.uint8, device=dev)
    rep = _Report()
    rc = _native.lib().v1c_jpeg_decode(dev.index, _stream_ptr(dev), data, len(data), out.data_ptr(), w * channels, channels, S, C.byref(rep))
    _check(rc, "v1c_jpeg_decode")
    _last.clear()
    _last.update(segments=rep.segments, subsequences=rep.subsequences, rounds=rep.rounds, path="device")
    return out


def imread_tensor(path: Any, *, device: Any = None, channels: int = 3, subseq_bits: int | None = None) -> torch.Tensor:
    """``decode_jpeg_tensor`` of a file"""
    return decode_jpeg_tensor(Path(path), device=device, channels=channels, subseq_bits=subseq_bits)


def last_decode_report() -> dict:
    """of the last successful decode: ``segments`` (stretches between restart markers), ``subsequences`` (lanes), ``rounds`` (launches
    until the entry states stood still) and ``path="device"``"""
    return dict(_last)


def read_inputs(items: Any, *, device: Any = None) -> list:
    """What ``device_decode=True`` does with its inputs: the ``.jpg`` / ``.jpeg`` paths among ``items`` become BGR device tensors; every
    other entry (arrays, tensors, other suffixes) is handed back as it is.  A file outside the device decoder's scope (progressive,
    ...) stays a path for the host reader; so does one that is damaged or cannot be read, with a warning, so that such a file meets
    the host reader's behaviour as it does without the option.  Any other error is raised."""
    out = []
    for q in items:
        if eligible(q):
            try:
                q = imread_tensor(q, device=device)
            except NotImplementedError as e:
                LOG.info(f"{q}: read on the host ({e})")
            except (CorruptJPEG, OSError) as e:
                LOG.warning(f"{q}: left to the host reader ({e})")
        out.append(q)
    return out


def eligible(path: Any) -> bool:
    """whether ``device_decode=True`` reads this input through the device decoder: a ``.jpg`` / ``.jpeg`` path"""
    return isinstance(path, (str, Path)) and Path(path).suffix.lower() in (".jpg", ".jpeg")


__all__ = ["decode_jpeg_tensor", "imread_tensor", "read_inputs", "last_decode_report", "eligible", "probe", "CorruptJPEG"]
