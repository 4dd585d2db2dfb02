"""The colours of one eye matched to the other's, on the device (``v1c_color_match_luts_async`` / ``v1c_apply_luts_async``;
INTEGRATION.md section 12 states the contract, tests/colormatch_ref.py restates it): per-channel histograms of both eyes over a joint
mask, a 256-entry table per colour channel that maps the target eye onto the reference eye (``mode="histogram"``: the distributions;
``mode="gain"``: one factor per channel), and the rewrite of the target eye through the tables.  Integer arithmetic from end to end.
Two cameras meter and white-balance on their own; in a headset the difference shows as binocular rivalry.

uint8 images only: a 65536-bin histogram of wide pixels does not fit the kernels' LDS and needs a design of its own."""
from __future__ import annotations

import ctypes as C
from typing import Any, NamedTuple

import torch

from . import _native

MODES = {"histogram": 0, "gain": 1}
REFERENCES = {"left": 0, "right": 1}
STATUS = {1: "too few pixels inside the joint mask", 2: "the target eye is black inside the mask (no gain)"}
REPORT_WORDS = 20


class ColorMatchParams(C.Structure):
    """``v1c_color_match_params`` (include/vr180_remap.h)"""

    _fields_ = [("mode", C.c_int32), ("reference", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32), ("max_shift", C.c_int32),
                ("min_pixels", C.c_int32)]


class ChannelReport(NamedTuple):
    left_first: int
    left_last: int
    right_first: int
    right_last: int
    gain: float  # g / 65536; 0.0 outside gain mode


class ColorMatchReport(NamedTuple):
    status: int
    n: int
    channels: tuple


def params(*, mode: str = "histogram", reference: str = "left", lo: int = 10, hi: int = 254, max_shift: int = 64,
           min_pixels: int = 1024) -> ColorMatchParams:
    if mode not in MODES:
        raise ValueError(f'mode must be "histogram" or "gain", not {mode!r}')
    if reference not in REFERENCES:
        raise ValueError(f'reference must be "left" or "right", not {reference!r}')
    return ColorMatchParams(MODES[mode], REFERENCES[reference], int(lo), int(hi), int(max_shift), int(min_pixels))


def _image_args(image: Any, who: str):
    from .remapper import _check_image_tensor

    if not isinstance(image, torch.Tensor) or not image.is_cuda:
        raise TypeError(f"{who}: a CUDA tensor is needed")
    if image.dtype != torch.uint8:  # (before any launch)
        raise TypeError(f"{who}: uint8 images only, not {image.dtype}")
    _check_image_tensor(image, "image")
    h, w, cn = (int(v) for v in image.shape)
    return h, w, cn, (image.stride(0) if h > 1 else w * cn)


def color_match_luts_tensor(left: torch.Tensor, right: torch.Tensor, *, workspace: torch.Tensor | None = None,
                            **prm: Any) -> tuple[torch.Tensor, torch.Tensor]:
    """The tables that map the target eye onto the reference eye: ``(luts, report)``, a ``(3, 256)`` uint8 and a ``(20,)`` int32 tensor,
    both left on the device.  Current stream, nothing synchronised; it can be captured into a graph (the workspace comes from torch's
    allocator, which keeps it alive with the graph; ``workspace``: a ``(2, 3, 256)`` int32 tensor of the caller's instead, which holds the
    histograms afterwards).  ``prm``: ``mode``, ``reference``, ``lo``, ``hi``, ``max_shift``, ``min_pixels``.  Neither eye is written.
    uint16 / float32 images raise TypeError before any launch."""
    from .remapper import _stream_ptr

    h, w, cn, pl = _image_args(left, "color_match_luts_tensor")
    h2, w2, cn2, pr = _image_args(right, "color_match_luts_tensor")
    if (h, w, cn) != (h2, w2, cn2) or left.device != right.device:
        raise ValueError("color_match_luts_tensor: the eyes must have one shape and one device")
    p = params(**prm)
    L = _native.lib()
    dev = left.device
    if workspace is None:
        workspace = torch.empty((2, 3, 256), dtype=torch.int32, device=dev)
    elif workspace.dtype != torch.int32 or workspace.numel() * 4 < int(L.v1c_color_match_workspace()) or not workspace.is_contiguous() \
            or workspace.device != dev:
        raise ValueError("color_match_luts_tensor: workspace must be a contiguous int32 tensor of 2 x 3 x 256 on the eyes' device")
    luts = torch.empty((3, 256), dtype=torch.uint8, device=dev)
    report = torch.empty(REPORT_WORDS, dtype=torch.int32, device=dev)
    rc = L.v1c_color_match_luts_async(dev.index, _stream_ptr(dev), left.data_ptr(), pl, right.data_ptr(), pr, h, w, cn, C.byref(p),
                                      workspace.data_ptr(), luts.data_ptr(), report.data_ptr())
    _native.check(rc, "v1c_color_match_luts_async")
    return luts, report


def apply_luts_tensor(image: torch.Tensor, luts: torch.Tensor, *, out: torch.Tensor | None = None) -> torch.Tensor:
    """``out[c] = luts[c][image[c]]`` on the colour channels, a fourth channel copied; ``out=None`` allocates, ``out=image`` rewrites in
    place.  One launch on the current stream.  The tables may come from another pair of the same shoot."""
    from .remapper import _stream_ptr

    h, w, cn, ps = _image_args(image, "apply_luts_tensor")
    if not isinstance(luts, torch.Tensor) or luts.dtype != torch.uint8 or luts.numel() != 768 or not luts.is_contiguous() \
            or luts.device != image.device:
        raise ValueError("apply_luts_tensor: luts must be a contiguous (3, 256) uint8 tensor on the image's device")
    if out is None:
        out = torch.empty((h, w, cn), dtype=torch.uint8, device=image.device)
    h2, w2, cn2, pd = _image_args(out, "apply_luts_tensor")
    if (h, w, cn) != (h2, w2, cn2) or out.device != image.device:
        raise ValueError("apply_luts_tensor: out must have the image's shape and device")
    dev = image.device
    rc = _native.lib().v1c_apply_luts_async(dev.index, _stream_ptr(dev), image.data_ptr(), ps, out.data_ptr(), pd, h, w, cn, luts.data_ptr())
    _native.check(rc, "v1c_apply_luts_async")
    return out


def match_eyes_tensors(left: torch.Tensor, right: torch.Tensor, *, out: torch.Tensor | None = None, reference: str = "left",
                       **prm: Any) -> torch.Tensor:
    """The eye that is not the ``reference`` rewritten through the tables of ``color_match_luts_tensor`` -- in place when ``out`` is None
    -- and returned.  The reference eye is never written.  Three launches on the current stream."""
    luts, _ = color_match_luts_tensor(left, right, reference=reference, **prm)
    target = right if reference == "left" else left
    return apply_luts_tensor(target, luts, out=target if out is None else out)


def color_match_report(report: torch.Tensor) -> ColorMatchReport:
    """The report record on the host.  Synchronises once."""
    r = [int(v) for v in report.cpu().tolist()]
    return ColorMatchReport(r[0], r[1], tuple(ChannelReport(*r[2 + 5 * c: 6 + 5 * c], r[6 + 5 * c] / 65536.0) for c in range(3)))
