"""JPEG files of device-resident results, encoded on the MI355X (``v1c_jpeg_encode``, csrc/kernels_jpeg.hip; a list of them in shared
launches: ``v1c_jpeg_encode_batch``, csrc/kernels_jpeg_batch.hip): colour conversion,
chroma downsampling, the forward DCT, quantisation, Huffman coding, byte stuffing and the restart markers are HIP kernels, only the
finished scan comes to the host, and the header segments (``v1c_jpeg_header``) and EOI are put around it here.

Baseline sequential JPEG with the standard tables, which every reader decodes -- not libjpeg's output byte for byte: the chroma
rounding differs and the file carries restart markers (INTEGRATION.md section 7 has the contract and the measured sizes;
``tests/jpg_ref.py`` restates the file).

``optimize=True`` (off by default) gives every image Huffman tables of its own, as ``IMWRITE_JPEG_OPTIMIZE`` and Pillow's
``optimize=True`` do on the host: the symbols are counted and the tables built on the device (``v1c_jpeg_encode_opt``,
``v1c_jpeg_encode_batch_opt``, csrc/kernels_jpeg_opt.hip) between two kernels of the same chain, so a call still synchronises twice;
the pixels a reader decodes are the same, the file is smaller (``tests/jpg_opt_ref.py`` restates it).
"""
from __future__ import annotations

import ctypes as C
import threading
from pathlib import Path
from typing import Any, Sequence

import torch

from . import _native
from .remapper import _stream_ptr

SUBSAMPLINGS = {"444": 0, "420": 2}  # V1C_JPEG_444 / V1C_JPEG_420
HEADER_MAX = 1024                    # V1C_JPEG_HEADER_MAX
DHT_MAX = 4 * (1 + 16 + 256)         # V1C_JPEG_DHT_MAX
HEADER_OPT_MAX = 2048                # V1C_JPEG_HEADER_OPT_MAX
# Bytes of page-locked memory a batch may land in at once (the sum of its images' v1c_jpeg_bound: 3.25 bytes per sample byte of a BGR
# image in 4:2:0, so 64 results of 2048 x 2048 would pin 1.3 GB); a longer list goes to the engine in several sub-lists.
PINNED_BUDGET = 1 << 30


class JpegImage(C.Structure):
    """``v1c_jpeg_image`` (include/vr180_remap.h)"""
    _fields_ = [("img", C.c_void_p), ("h", C.c_int), ("w", C.c_int), ("pitch", C.c_int64), ("cn", C.c_int), ("quality", C.c_int),
                ("subsampling", C.c_int), ("restart_mcus", C.c_int), ("out_host", C.c_void_p), ("capacity", C.c_uint64), ("size", C.c_uint64)]


class JpegImageOpt(C.Structure):
    """``v1c_jpeg_image_opt`` (include/vr180_remap.h)"""
    _fields_ = JpegImage._fields_ + [("optimize", C.c_int), ("dht_size", C.c_uint32), ("dht", C.c_uint8 * DHT_MAX)]


def default_restart_mcus(height: int, width: int, channels: int, subsampling: str = "420") -> int:
    """MCUs per restart interval when the caller names none: one MCU row, so that the intervals follow the image's rows (a decoder
    can start at any of them) and an 8192 x 4096 frame has 256 (4:2:0) or 512 (4:4:4) of them.  The kernels' work does not depend
    on it: every lane's work is bounded whatever the interval."""
    m = 16 if (channels != 1 and subsampling == "420") else 8
    return min(65535, -(-width // m))


# Per calling thread (as remapper._TLS keeps the last plans per thread):
#   .pinned: {device index: the page-locked buffer the thread's scans land in}, grown on demand and kept until the thread ends.  The
#            engine call releases the GIL and the callers read views of the buffer after it, so a buffer shared between threads would
#            hand one thread another's scan; the lossless entries (jpeg_transcode_device._run_outputs) land in the same buffer.
#   .encode_batch: the report of the thread's last batch (last_encode_batch_report)
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


def _params(t: torch.Tensor, quality: int, subsampling: str, restart_mcus: int | None) -> tuple:
    """the checked arguments of one image: (tensor as the engine takes it, h, w, cn, quality, subsampling code, restart interval)"""
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
    return t, h, w, cn, quality, SUBSAMPLINGS[subsampling], restart


def _header(h: int, w: int, cn: int, quality: int, sub: int, restart: int) -> bytes:
    head = (C.c_uint8 * HEADER_MAX)()
    n = _native.lib().v1c_jpeg_header(h, w, cn, quality, sub, restart, head, HEADER_MAX)
    if n < 0:
        _native.check(int(n), "v1c_jpeg_header")
    return bytes(head[:n])


def _header_opt(h: int, w: int, cn: int, quality: int, sub: int, restart: int, dht: Any, dht_size: int) -> bytes:
    head = (C.c_uint8 * HEADER_OPT_MAX)()
    n = _native.lib().v1c_jpeg_header_opt(h, w, cn, quality, sub, restart, dht, dht_size, head, HEADER_OPT_MAX)
    if n < 0:
        _native.check(int(n), "v1c_jpeg_header_opt")
    return bytes(head[:n])


def _parts(t: torch.Tensor, quality: int, subsampling: str, restart_mcus: int | None, optimize: bool = False) -> list:
    t, h, w, cn, quality, sub, restart = _params(t, quality, subsampling, restart_mcus)
    lib = _native.lib()
    cap = int(lib.v1c_jpeg_bound(h, w, cn, sub, restart))
    dev = t.device
    buf = _host_buffer(dev, cap)
    size = C.c_uint64(0)
    pitch = t.stride(0) if h > 1 else w * cn
    if optimize:
        dht, dht_size = (C.c_uint8 * DHT_MAX)(), C.c_uint32(0)
        rc = lib.v1c_jpeg_encode_opt(dev.index, _stream_ptr(dev), t.data_ptr(), h, w, pitch, cn, quality, sub, restart, buf.data_ptr(), buf.numel(),
                                     C.byref(size), dht, C.byref(dht_size))
        _native.check(rc, "v1c_jpeg_encode_opt")
        return [_header_opt(h, w, cn, quality, sub, restart, dht, dht_size.value), buf.numpy()[:size.value], b"\xff\xd9"]
    head = _header(h, w, cn, quality, sub, restart)
    rc = lib.v1c_jpeg_encode(dev.index, _stream_ptr(dev), t.data_ptr(), h, w, pitch, cn, quality, sub, restart, buf.data_ptr(), buf.numel(),
                             C.byref(size))
    _native.check(rc, "v1c_jpeg_encode")
    return [head, buf.numpy()[:size.value], b"\xff\xd9"]


def encode_jpeg_tensor(t: torch.Tensor, *, quality: int = 95, subsampling: str = "420", restart_mcus: int | None = None,
                       optimize: bool = False) -> bytes:
    """JPEG bytes of a CUDA ``uint8`` tensor ``(H, W[, C])`` in cv2 channel order (C 1: greyscale, 3: YCbCr, 4: alpha dropped), encoded
    on the device on the current stream.  ``quality``: 1 ... 100, the IJG rule (95: the host writer's).  ``subsampling``: ``"420"``
    (cv2's and Pillow's at that quality) or ``"444"``.  ``restart_mcus``: MCUs per restart interval, 1 ... 65535
    (``default_restart_mcus``: one MCU row).  ``optimize``: Huffman tables built for this image on the device in place of the Annex K
    tables (a smaller file of the same pixels; the call still synchronises twice).  Two calls give identical bytes."""
    return b"".join(bytes(p) for p in _parts(t, quality, subsampling, restart_mcus, bool(optimize)))


def imwrite_jpeg_tensor(path: Any, t: torch.Tensor, *, quality: int = 95, subsampling: str = "420", restart_mcus: int | None = None,
                        optimize: bool = False) -> None:
    """``encode_jpeg_tensor`` into a file (the scan goes from the page-locked buffer to the file without a copy in between)"""
    with open(path, "wb") as f:
        for part in _parts(t, quality, subsampling, restart_mcus, bool(optimize)):
            f.write(part)


def last_encode_batch_report() -> dict:
    """``{"chunks": ..., "sizes": [...]}`` of the calling thread's last ``encode_jpeg_tensors`` / ``imwrite_jpeg_tensors`` call: the chunks
    the engine ran (two synchronisations each) over all sub-lists, and every image's scan size"""
    last = getattr(_TLS, "encode_batch", {"chunks": 0, "sizes": []})
    return {"chunks": last["chunks"], "sizes": list(last["sizes"])}


def _per_image(value: Any, n: int, name: str) -> list:
    if isinstance(value, (str, bytes)) or not isinstance(value, Sequence):
        return [value] * n
    if len(value) != n:
        raise ValueError(f"{name} has {len(value)} entries for {n} images")
    return list(value)


def sub_lists(bounds: Sequence[int], budget: int | None = None) -> list[tuple[int, int]]:
    """the ``[lo, hi)`` sub-lists a batch goes to the engine in: images in order while the sum of their bounds stays within the budget
    of page-locked bytes (``PINNED_BUDGET``, or the largest single bound where that is larger); each holds at least one image"""
    budget = max(PINNED_BUDGET if budget is None else int(budget), max(bounds, default=0))
    out, lo, total = [], 0, 0
    for i, b in enumerate(bounds):
        if i > lo and total + b > budget:
            out.append((lo, i))
            lo, total = i, 0
        total += b
    if len(bounds) > lo:
        out.append((lo, len(bounds)))
    return out


def _batch_parts(tensors: Sequence[torch.Tensor], quality: Any, subsampling: Any, restart_mcus: Any, workspace_budget: int | None,
                 optimize: Any = False):
    """yields (index, [header, scan, EOI]) of every image, sub-list by sub-list; a scan is a view of the calling thread's page-locked
    buffer that holds until the thread encodes the next sub-list"""
    n = len(tensors)
    qs, ss, rs = _per_image(quality, n, "quality"), _per_image(subsampling, n, "subsampling"), _per_image(restart_mcus, n, "restart_mcus")
    opts = [bool(o) for o in _per_image(optimize, n, "optimize")]
    report = _TLS.encode_batch = {"chunks": 0, "sizes": []}
    if n == 0:
        return
    params = [_params(t, q, s, r) for t, q, s, r in zip(tensors, qs, ss, rs)]
    devs = {p[0].device for p in params}
    if len(devs) != 1:
        raise ValueError(f"the images of a batch must be on one device, not on {sorted(str(d) for d in devs)}")
    dev = devs.pop()
    if workspace_budget is not None and int(workspace_budget) < 0:
        raise ValueError("workspace_budget must not be negative")
    lib = _native.lib()
    bounds = [int(lib.v1c_jpeg_bound(h, w, cn, sub, restart)) for _, h, w, cn, _, sub, restart in params]
    sizes = []
    for lo, hi in sub_lists(bounds):
        buf = _host_buffer(dev, sum(bounds[lo:hi]))
        # a sub-list without an optimising image goes to the entry it went to before there was the option
        some = any(opts[lo:hi])
        images = ((JpegImageOpt if some else JpegImage) * (hi - lo))()
        at = 0
        for k in range(lo, hi):
            t, h, w, cn, q, sub, restart = params[k]
            fields = (t.data_ptr(), h, w, t.stride(0) if h > 1 else w * cn, cn, q, sub, restart, buf.data_ptr() + at, bounds[k], 0)
            images[k - lo] = JpegImageOpt(*fields, int(opts[k])) if some else JpegImage(*fields)
            at += bounds[k]
        chunks = C.c_uint32(0)
        entry = "v1c_jpeg_encode_batch_opt" if some else "v1c_jpeg_encode_batch"
        rc = getattr(lib, entry)(dev.index, _stream_ptr(dev), hi - lo, images, int(workspace_budget or 0), C.byref(chunks))
        _native.check(rc, entry)
        report["chunks"] += chunks.value
        host, at = buf.numpy(), 0
        for k in range(lo, hi):
            _, h, w, cn, q, sub, restart = params[k]
            size = int(images[k - lo].size)
            sizes.append(size)
            head = (_header_opt(h, w, cn, q, sub, restart, images[k - lo].dht, int(images[k - lo].dht_size)) if opts[k]
                    else _header(h, w, cn, q, sub, restart))
            yield k, [head, host[at:at + size], b"\xff\xd9"]
            at += bounds[k]
    report["sizes"] = sizes


def encode_jpeg_tensors(tensors: Sequence[torch.Tensor], *, quality: Any = 95, subsampling: Any = "420", restart_mcus: Any = None,
                        workspace_budget: int | None = None, optimize: Any = False) -> list[bytes]:
    """``encode_jpeg_tensor`` of every tensor of a list in shared launches (``v1c_jpeg_encode_batch``, csrc/kernels_jpeg_batch.hip): every
    file is byte for byte the single call's.  ``quality``, ``subsampling``, ``restart_mcus`` and ``optimize`` are each one value for all
    images or a sequence of the list's length (a list may mix optimising and plain images; the count of synchronisations does not
    change with it); the images may differ in size and channels but lie on one device; runs on the current stream.  The
    engine cuts the list into chunks of at most ``workspace_budget`` bytes of device workspace (``None``: 1 GiB), each of which
    synchronises twice; a list whose summed ``v1c_jpeg_bound`` passes ``PINNED_BUDGET`` goes to the engine in several sub-lists
    (``sub_lists``), which multiplies that count a second time.  ``last_encode_batch_report()`` tells what ran."""
    out: list[bytes] = [b""] * len(tensors)
    for k, parts in _batch_parts(tensors, quality, subsampling, restart_mcus, workspace_budget, optimize):
        out[k] = b"".join(bytes(p) for p in parts)
    return out


def imwrite_jpeg_tensors(paths: Sequence[Any], tensors: Sequence[torch.Tensor], *, quality: Any = 95, subsampling: Any = "420",
                         restart_mcus: Any = None, workspace_budget: int | None = None, optimize: Any = False) -> None:
    """``encode_jpeg_tensors`` into files (every scan goes from the page-locked buffer to its file without a copy in between)"""
    if len(paths) != len(tensors):
        raise ValueError(f"{len(paths)} paths for {len(tensors)} images")
    for k, parts in _batch_parts(tensors, quality, subsampling, restart_mcus, workspace_budget, optimize):
        with open(paths[k], "wb") as f:
            for part in parts:
                f.write(part)


def eligible(path: Any, result: Any) -> bool:
    """whether ``device_jpeg=True`` writes this result through the device encoder: a ``.jpg`` / ``.jpeg`` path and a uint8 device tensor"""
    return (isinstance(path, (str, Path)) and Path(path).suffix.lower() in (".jpg", ".jpeg") and isinstance(result, torch.Tensor)
            and result.is_cuda and result.dtype == torch.uint8)


__all__ = ["encode_jpeg_tensor", "imwrite_jpeg_tensor", "encode_jpeg_tensors", "imwrite_jpeg_tensors", "last_encode_batch_report",
           "default_restart_mcus", "eligible"]
