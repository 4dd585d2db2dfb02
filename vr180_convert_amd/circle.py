"""The image circle of a fisheye frame from its rim, fitted on the device (``v1c_fit_circle*``; INTEGRATION.md section 11 states the
contract, tests/circle_ref.py restates it): centre and radius from the first lit run at both ends of every row and column, an algebraic
circle fit of their integer moment sums and four trimmed refits.  It holds where ``get_radius`` -- one scan of the centre row or column
about an assumed centre -- does not: a lens axis off the sensor's centre, the halves of a side-by-side frame, a dark object on the rim,
a circle the frame clips."""
from __future__ import annotations

import ctypes as C
from typing import Any, NamedTuple

import numpy as np
import torch

from . import _abi, _native

DEFAULT_TOL16 = (128, 48, 24, 24)  # 8, 3, 1.5 and 1.5 px
STATUS = {1: "too few rim points", 2: "the rim points do not span a circle (singular system)", 3: "radius or centre out of range"}


class CircleParams(C.Structure):
    """``v1c_circle_params`` (include/vr180_remap.h)"""

    _fields_ = [("threshold", C.c_int32), ("run", C.c_int32), ("rounds", C.c_int32), ("min_points", C.c_int32), ("tol16", C.c_int32 * 8)]


class CirclePoint(C.Structure):
    """``v1c_circle_point``"""

    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("selected", C.c_int32)]


class Circle(NamedTuple):
    cx: float
    cy: float
    radius: float
    n_rim: int
    n_used: int
    rms: float


def params(*, threshold: int = 10, run: int = 4, rounds: int | None = None, min_points: int = 8, tol16: Any = None) -> CircleParams:
    """``tol16``: the selection tolerance of every refit in 1/16 px (default 128, 48, 24, 24); ``rounds`` defaults to its length"""
    tol = [int(t) for t in (DEFAULT_TOL16 if tol16 is None else tol16)]
    rounds = len(tol) if rounds is None else int(rounds)
    if not 0 <= rounds <= 8 or len(tol) < rounds:
        raise ValueError("rounds must be 0..8 with one tolerance each")
    tol = tol[:rounds] + [0] * (8 - rounds)
    return CircleParams(int(threshold), int(run), rounds, int(min_points), (C.c_int32 * 8)(*tol))


def _image_args(image: torch.Tensor, who: str):
    from .remapper import _check_image_tensor

    if not isinstance(image, torch.Tensor) or not image.is_cuda:
        raise TypeError(f"{who}: a CUDA tensor is needed")
    if image.dtype not in (torch.uint8, torch.uint16):  # (before any launch, as auto_radius_tensor)
        raise TypeError(f"{who}: uint8 or uint16 images only, not {image.dtype}")
    _check_image_tensor(image, "image")
    h, w, cn = (int(v) for v in image.shape)
    depth = _abi.DEPTH_8U if image.dtype == torch.uint8 else _abi.DEPTH_16U
    pitch = (image.stride(0) if h > 1 else w * cn) * image.element_size()
    return h, w, cn, depth, pitch


def fit_circle_tensor(image: torch.Tensor, *, threshold: int = 10, **prm: Any) -> torch.Tensor:
    """The fit of one ``(H, W, C)`` uint8 / uint16 image on the device: eight float64 ``(cx, cy, r, status, n_rim, n_used, rms, 0)`` left
    there (``v1c_fit_circle_async``).  Current stream, four launches, nothing synchronised; it can be captured into a graph (the
    workspace comes from torch's allocator, which keeps it alive with the graph).  ``prm``: ``run``, ``rounds``, ``min_points``,
    ``tol16``.  float32 images raise TypeError before any launch."""
    from .remapper import _stream_ptr

    h, w, cn, depth, pitch = _image_args(image, "fit_circle_tensor")
    p = params(threshold=threshold, **prm)
    L = _native.lib()
    dev = image.device
    ws = torch.empty(int(L.v1c_fit_circle_workspace(h, w)), dtype=torch.uint8, device=dev)
    out = torch.empty(8, dtype=torch.float64, device=dev)
    rc = L.v1c_fit_circle_async(dev.index, _stream_ptr(dev), image.data_ptr(), h, w, pitch, cn, depth, C.byref(p), ws.data_ptr(), out.data_ptr())
    _native.check(rc, "v1c_fit_circle_async")
    return out


def fit_circle_raw(image: Any, *, device: Any = None, points: bool = False, threshold: int = 10, **prm: Any):
    """``v1c_fit_circle``: the eight doubles on the host (one synchronisation) and, with ``points``, the ``(n, 3)`` int32 rim points
    ``(x, y, selected)`` in order.  numpy images go up as ``_to_device`` takes them.  Nothing is raised for a non-zero status."""
    from .remapper import _device, _stream_ptr, _to_device

    if not (isinstance(image, torch.Tensor) and image.is_cuda):
        a = image if isinstance(image, torch.Tensor) else np.asarray(image)
        if a.dtype not in (np.uint8, np.uint16, torch.uint8, torch.uint16):
            raise TypeError(f"fit_circle: uint8 or uint16 images only, not {a.dtype}")
        image = _to_device(image, _device(device))
    h, w, cn, depth, pitch = _image_args(image, "fit_circle")
    p = params(threshold=threshold, **prm)
    L = _native.lib()
    dev = image.device
    ws = torch.empty(int(L.v1c_fit_circle_workspace(h, w)), dtype=torch.uint8, device=dev)
    out = np.zeros(8, np.float64)
    cap = 2 * (h + w)
    pts = np.zeros((cap, 3), np.int32) if points else None
    n = C.c_int32(0)
    rc = L.v1c_fit_circle(dev.index, _stream_ptr(dev), image.data_ptr(), h, w, pitch, cn, depth, C.byref(p), ws.data_ptr(), out.ctypes.data,
                          pts.ctypes.data if points else None, cap if points else 0, C.byref(n) if points else None)
    _native.check(rc, "v1c_fit_circle")
    return (out, pts[: n.value]) if points else out


def fit_circle(image: Any, *, device: Any = None, threshold: int = 10, **prm: Any) -> Circle:
    """Centre and radius of the image circle of one image (numpy array or tensor, uint8 / uint16, 1, 3 or 4 channels), in source
    pixels.  Raises ``ValueError("no image circle found: ...")`` where the fit ends in a status: an all-black or all-lit frame, rim
    points on one line."""
    out = fit_circle_raw(image, device=device, threshold=threshold, **prm)
    if out[3] != 0:
        raise ValueError(f"no image circle found: {STATUS.get(int(out[3]), 'status %d' % int(out[3]))} "
                         f"({int(out[4])} rim points, {int(out[5])} in the last fit)")
    return Circle(float(out[0]), float(out[1]), float(out[2]), int(out[4]), int(out[5]), float(out[6]))


def round_center(cx: float, cy: float) -> tuple[float, float]:
    """a fitted centre on the 1/4 px grid the entry points lower it on: the fit is not better than that on real rims, and the frames
    of one rig then share a plan"""
    return (float(np.floor(cx * 4.0 + 0.5) / 4.0), float(np.floor(cy * 4.0 + 0.5) / 4.0))


def round_radius(r: float) -> float:
    """a fitted radius on get_radius's own grid of 1/2 px"""
    return float(np.floor(r * 2.0 + 0.5) / 2.0)
