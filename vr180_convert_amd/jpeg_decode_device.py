"""JPEG files decoded on the MI355X into device tensors (``v1c_jpeg_decode``, csrc/kernels_jpegdec.hip): only the file's bytes cross
PCIe.  The host parses the markers and walks the scan's 0xFF bytes; unstuffing, Huffman decoding -- parallel over subsequences of
the scan whose entry states are found by iteration --, the DC scan, dequantisation, the inverse DCT, chroma upsampling and colour
conversion are HIP kernels.

Baseline and extended sequential Huffman files (SOF0 / SOF1, 8-bit) of one component or of three in 4:4:4, 4:2:2 or 4:2:0, with any
tables and any restart interval or none; the pixels are libjpeg's default decode (INTEGRATION.md section 8 has the contract,
``tests/jpgdec_ref.py`` restates it).  Anything else raises ``NotImplementedError`` from a host-only parse, a damaged file
``ValueError``: nothing falls back silently.

``progressive=True`` adds progressive Huffman files (SOF2) of the same components and samplings with any legal scan script that
brings every coefficient to full precision: every scan is decoded as the one scan of a sequential file is, into one coefficient store
(``v1c_jpeg_prog_decode``, csrc/kernels_jpegprog.hip; ``tests/jpgprog_ref.py`` restates the contract).  Off by default: AC refinement
scans take about one round per subsequence, so large files without restart markers decode far slower than on the host (DESIGN.md
section 18).
"""
from __future__ import annotations

import ctypes as C
import logging
import threading
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


class _Last(threading.local):
    """the report of the calling thread's last call: every thread sees a dict of its own (as remapper._TLS keeps the last plans per
    thread), so a thread that asks what its call did is not told about another thread's"""

    def __init__(self) -> None:
        self.report: dict = {}

    def clear(self) -> None:
        self.report = {}

    def update(self, **kw: Any) -> None:
        self.report.update(kw)

    def get(self) -> dict:
        return dict(self.report)


LOG = logging.getLogger(__name__)
_last = _Last()
_last_batch = _Last()


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


def probe_progressive(data_or_path: Any) -> tuple[int, int, int, int]:
    """(height, width, components, scans) of a PROGRESSIVE file the device decodes (``decode_jpeg_tensor(..., progressive=True)``), by
    the host-only parse of all its scans; ``NotImplementedError`` -- for a sequential file too -- / ``CorruptJPEG`` otherwise"""
    data = _bytes_of(data_or_path)
    info = _abi.JpegProgInfo()
    _check(_native.lib().v1c_jpeg_prog_info(data, len(data), C.byref(info)), "v1c_jpeg_prog_info")
    return info.height, info.width, info.components, info.scans


def _decode_progressive(data: bytes, device: Any, channels: int, S: int) -> torch.Tensor:
    h, w, nc, scans = probe_progressive(data)
    if channels == 1 and nc != 1:
        raise ValueError("channels=1 takes a grey file")
    dev = _device(device)
    out = torch.empty((h, w) if channels == 1 else (h, w, 3), dtype=torch.uint8, device=dev)
    rep = _abi.JpegProgReport()
    per_scan = (C.c_uint32 * scans)()
    rc = _native.lib().v1c_jpeg_prog_decode(dev.index, _stream_ptr(dev), data, len(data), out.data_ptr(), w * channels, channels, S,
                                            C.byref(rep), per_scan, scans)
    _check(rc, "v1c_jpeg_prog_decode")
    _last.clear()
    _last.update(segments=rep.segments, subsequences=rep.subsequences, rounds=rep.rounds, path="device", scans=rep.scans,
                 scan_rounds=list(per_scan))
    return out


def decode_jpeg_tensor(data_or_path: Any, *, device: Any = None, channels: int = 3, subseq_bits: int | None = None,
                       progressive: bool = False) -> torch.Tensor:
    """A JPEG file (its bytes, or a path) as a CUDA ``uint8`` tensor in cv2 channel order, decoded on the device on the current
    stream: ``(H, W, 3)`` BGR (a grey file replicated, as ``cv2.imread`` does), or ``(H, W)`` with ``channels=1`` for a grey file.
    ``subseq_bits``: bits of the scan one lane decodes, a multiple of 32 from 256 (None: the engine's default); the pixels do not
    depend on it.  EXIF orientation is not applied.  Raises ``NotImplementedError`` for a file outside the device decoder's scope and
    ``CorruptJPEG`` (a ``ValueError``) for a damaged one; ``last_decode_report()`` tells what the call did.
    ``progressive=True``: a progressive Huffman file (SOF2) of the same components and samplings, with any legal scan script that
    brings every coefficient to full precision, is decoded on the device too, scan by scan (``v1c_jpeg_prog_decode``); sequential
    files are decoded exactly as without it.  Off, such a file is refused as ever."""
    if channels not in (1, 3):
        raise ValueError("channels must be 1 or 3")
    S = 0 if subseq_bits is None else int(subseq_bits)
    if S and (S % 32 or S < 256):
        raise ValueError("subseq_bits must be a multiple of 32, at least 256")
    data = _bytes_of(data_or_path)
    try:
        h, w, nc = probe(data)
    except NotImplementedError:
        if not progressive or not _is_progressive(data):
            raise
        return _decode_progressive(data, device, channels, S)
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


def _is_progressive(data: bytes) -> bool:
    """whether the host-only parse of the progressive decoder is the one to ask: the file's frame header is SOF2"""
    pos = 2
    while pos + 4 <= len(data) and data[pos] == 0xFF:
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
        elif m == 0x01 or 0xD0 <= m <= 0xD8:
            pos += 2
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return m == 0xC2
        elif m in (0xD9, 0xDA):
            return False
        else:
            pos += 2 + (data[pos + 2] << 8 | data[pos + 3])
    return False


def imread_tensor(path: Any, *, device: Any = None, channels: int = 3, subseq_bits: int | None = None,
                  progressive: bool = False) -> torch.Tensor:
    """``decode_jpeg_tensor`` of a file"""
    return decode_jpeg_tensor(Path(path), device=device, channels=channels, subseq_bits=subseq_bits, progressive=progressive)


def last_decode_report() -> dict:
    """of the calling thread's last successful decode: ``segments`` (stretches between restart markers), ``subsequences`` (lanes), ``rounds`` (launches
    until the entry states stood still) and ``path="device"``; after a progressive file the three are summed over its scans, and
    ``scans`` and ``scan_rounds`` (a list) are there too"""
    return _last.get()


def _error_of(rc: int, what: str, msg: str) -> Exception:
    """the exception ``_check`` raises for a return code, as an object"""
    if rc == _abi.E_CORRUPT:
        return CorruptJPEG(f"{what}: {msg}")
    if rc == _abi.E_INVALID:
        return ValueError(f"{what}: {msg}")
    if rc == _abi.E_UNSUPPORTED:
        return NotImplementedError(f"{what}: {msg}")
    return _native.EngineError(f"{what}: {msg} (code {rc})")


def decode_jpeg_tensors(items: Any, *, device: Any = None, channels: int = 3, subseq_bits: int | None = None,
                        max_workspace_bytes: int | None = None, errors: str = "raise") -> list:
    """``decode_jpeg_tensor`` of every item (bytes or paths) in ONE call of the engine (``v1c_jpeg_decode_batch``): the files share
    their kernel launches and their synchronisation rounds, so the list costs the rounds of its slowest file and not the sum.  The
    tensors, and what a file is refused for, are those of ``decode_jpeg_tensor`` file by file.  ``max_workspace_bytes``: the files are
    taken in order into chunks whose device workspace stays under it (None: the engine's default; a larger file is a chunk of its
    own).  ``errors="raise"``: after the batch ran, the first failing file's exception is raised; ``errors="return"``: every failing
    file's exception object stands in its place in the list and the others are decoded.  ``last_batch_report()`` tells what the call
    did; ``last_decode_report()`` is left alone."""
    if errors not in ("raise", "return"):
        raise ValueError('errors must be "raise" or "return"')
    if channels not in (1, 3):
        raise ValueError("channels must be 1 or 3")
    S = 0 if subseq_bits is None else int(subseq_bits)
    if S and (S % 32 or S < 256):
        raise ValueError("subseq_bits must be a multiple of 32, at least 256")
    items = list(items)
    n = len(items)
    out: list = [None] * n
    data: list = [b""] * n
    for i, q in enumerate(items):
        try:
            data[i] = _bytes_of(q)
            h, w, nc = probe(data[i])
            if channels == 1 and nc != 1:
                raise ValueError("channels=1 takes a grey file")
            out[i] = (h, w)
        except (NotImplementedError, ValueError, OSError) as e:  # (what decode_jpeg_tensor raises before it looks for a device)
            out[i] = e
    live = [i for i in range(n) if not isinstance(out[i], Exception)]
    reports: list = [None] * n
    rounds = C.c_uint32(0)
    chunks = 0
    if live:
        dev = _device(device)
        m = len(live)
        for i in live:
            h, w = out[i]
            out[i] = torch.empty((h, w) if channels == 1 else (h, w, 3), dtype=torch.uint8, device=dev)
        files = (C.c_char_p * m)(*[data[i] for i in live])
        sizes = (C.c_uint64 * m)(*[len(data[i]) for i in live])
        outs = (C.c_void_p * m)(*[out[i].data_ptr() for i in live])
        pitches = (C.c_int64 * m)(*[out[i].shape[1] * channels for i in live])
        cns = (C.c_int * m)(*([channels] * m))
        status = (C.c_int * m)()
        reps = (_Report * m)()
        budget = 0 if max_workspace_bytes is None else int(max_workspace_bytes)
        rc = _native.lib().v1c_jpeg_decode_batch(dev.index, _stream_ptr(dev), m, files, sizes, outs, pitches, cns, S, budget, status, reps,
                                                 C.byref(rounds))
        _check(rc, "v1c_jpeg_decode_batch")
        for k, i in enumerate(live):
            reports[i] = dict(segments=reps[k].segments, subsequences=reps[k].subsequences, rounds=reps[k].rounds, path="device")
            if status[k] != _abi.OK:
                what = (f"the entropy-coded data is damaged at bit {reps[k].error_pos} of the unstuffed scan" if status[k] == _abi.E_CORRUPT
                        else f"status {status[k]}")
                out[i] = _error_of(status[k], "v1c_jpeg_decode_batch", f"file {i}: {what}")
                reports[i] = None
        chunks = max((reps[k].reserved + 1 for k in range(m) if reps[k].subsequences), default=0)  # (reserved: the file's chunk)
    _last_batch.clear()
    _last_batch.update(batch_rounds=int(rounds.value), chunks=int(chunks), files=reports)
    if errors == "raise":
        for o in out:
            if isinstance(o, Exception):
                raise o
    return out


def imread_tensors(paths: Any, *, device: Any = None, channels: int = 3, subseq_bits: int | None = None,
                   max_workspace_bytes: int | None = None, errors: str = "raise") -> list:
    """``decode_jpeg_tensors`` of files"""
    return decode_jpeg_tensors([Path(p) for p in paths], device=device, channels=channels, subseq_bits=subseq_bits,
                               max_workspace_bytes=max_workspace_bytes, errors=errors)


def last_batch_report() -> dict:
    """of the calling thread's last ``decode_jpeg_tensors`` call: ``batch_rounds`` (round launches, summed over the chunks), ``chunks`` and ``files``, per
    file the dict ``last_decode_report()`` gives after a single call, or None for a file that was not decoded"""
    return _last_batch.get()


def read_inputs(items: Any, *, device: Any = None, batch: bool = False, progressive: bool = False) -> list:
    """What ``device_decode=True`` does with its inputs: the ``.jpg`` / ``.jpeg`` paths among ``items`` become BGR device tensors; every
    other entry (arrays, tensors, other suffixes) is handed back as it is.  A file outside the device decoder's scope (progressive,
    ...) stays a path for the host reader; so does one that is damaged or cannot be read, with a warning, so that such a file meets
    the host reader's behaviour as it does without the option.  Any other error is raised.  ``batch=True`` (``device_decode="batch"``):
    the same outcomes and log lines from one ``imread_tensors`` call over all the eligible paths.  ``progressive=True``
    (``device_decode_progressive``): a progressive file stays on the device too -- under ``batch`` by a single call of its own behind
    the batch, which keeps refusing it."""
    if batch:
        items = list(items)
        at = [i for i, q in enumerate(items) if eligible(q)]
        got = imread_tensors([items[i] for i in at], device=device, errors="return") if at else []
        for i, t in zip(at, got):
            if isinstance(t, NotImplementedError) and progressive:
                try:
                    t = imread_tensor(items[i], device=device, progressive=True)
                except (NotImplementedError, CorruptJPEG, OSError) as e:
                    t = e
            if isinstance(t, NotImplementedError):
                LOG.info(f"{items[i]}: read on the host ({t})")
            elif isinstance(t, (CorruptJPEG, OSError)):
                LOG.warning(f"{items[i]}: left to the host reader ({t})")
            elif isinstance(t, Exception):
                raise t
            else:
                items[i] = t
        return items
    out = []
    for q in items:
        if eligible(q):
            try:
                q = imread_tensor(q, device=device, progressive=progressive)
            except NotImplementedError as e:
                LOG.info(f"{q}: read on the host ({e})")
            except (CorruptJPEG, OSError) as e:
                LOG.warning(f"{q}: left to the host reader ({e})")
        out.append(q)
    return out


def eligible(path: Any) -> bool:
    """whether ``device_decode=True`` reads this input through the device decoder: a ``.jpg`` / ``.jpeg`` path"""
    return isinstance(path, (str, Path)) and Path(path).suffix.lower() in (".jpg", ".jpeg")


__all__ = ["decode_jpeg_tensor", "imread_tensor", "decode_jpeg_tensors", "imread_tensors", "read_inputs", "last_decode_report",
           "last_batch_report", "eligible", "probe", "probe_progressive", "CorruptJPEG"]
