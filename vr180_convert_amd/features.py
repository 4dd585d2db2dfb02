"""Feature matching of the two eyes on the MI355X: ``--automatch devfm[scale]``, the calibration front end that works without OpenCV.

``match_points_device`` takes the place of ``calibration_cv.match_points`` (cv2.AKAZE + BFMatcher, reference remapper.py:194-248) and
returns the same 7-tuple, so that ``match_lr`` -> ``rotation_match_robust`` -> ``calibration_rotators`` run unchanged behind it.  It is
NOT AKAZE: a single-scale, oriented binary-feature pipeline (luma + block resampling, binomial smoothing, FAST-9 scores inside the image
circle, NMS + a per-cell grid + an N_max cap, steered 256-bit descriptors, mutual-best Hamming matching with a ratio test), every stage
integer arithmetic on the device (``v1c_feat_detect`` / ``v1c_feat_match``, csrc/kernels_feat.hip) and restated in NumPy by
``tests/feat_ref.py``.  INTEGRATION.md section 5 has the contract.

Inputs are uint8 (H, W[, C]) images, C 1 / 3 / 4 (BGR(A)), as numpy arrays or CUDA tensors; uint16 / float32 raise ``TypeError``.
"""
from __future__ import annotations

import ctypes as C
from typing import Any

import numpy as np
import torch

from . import _native
from .remapper import _device, _stream_ptr, get_radius_smart

# the defaults of v1c_feat_params (include/vr180_remap.h); `ratio` = (num, den): kept iff den * d1 <= num * d2
DEFAULTS = {"fast_threshold": 20, "margin": 19, "cell": 32, "per_cell": 2, "max_keypoints": 8192, "max_distance": 64, "ratio": (3, 4)}
# columns of a keypoint array: working-scale pixel, FAST-9 score, orientation sector, twice the source block's centre (original pixels)
KP_FIELDS = ("x", "y", "score", "bin", "src_x2", "src_y2")


class FeatParams(C.Structure):
    _fields_ = [("scale", C.c_double), ("radius", C.c_double), ("fast_threshold", C.c_int32), ("margin", C.c_int32),
                ("cell", C.c_int32), ("per_cell", C.c_int32), ("max_keypoints", C.c_int32), ("max_distance", C.c_int32),
                ("ratio_num", C.c_int32), ("ratio_den", C.c_int32)]


def params(scale: float = 1.0, radius: float = 1.0, **overrides: Any) -> FeatParams:
    unknown = set(overrides) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown feature parameter(s) {sorted(unknown)}; known: {sorted(DEFAULTS)}")
    p = {**DEFAULTS, **overrides}
    num, den = p["ratio"]
    return FeatParams(float(scale), float(radius), int(p["fast_threshold"]), int(p["margin"]), int(p["cell"]), int(p["per_cell"]),
                      int(p["max_keypoints"]), int(p["max_distance"]), int(num), int(den))


def _image_tensor(image: Any, dev: torch.device) -> torch.Tensor:
    if isinstance(image, torch.Tensor):
        if image.dtype != torch.uint8:
            raise TypeError(f"feature matching takes uint8 images only, not {image.dtype}")
        t = image if image.device == dev else image.to(dev)
    else:
        a = np.asarray(image)
        if a.dtype != np.uint8:
            raise TypeError(f"feature matching takes uint8 images only, not {a.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if t.dim() == 2:
        t = t[..., None]
    if t.dim() != 3 or t.shape[2] not in (1, 3, 4):
        raise ValueError(f"feature matching takes (H, W[, C]) images with C 1, 3 or 4, not {tuple(t.shape)}")
    if (t.shape[2] > 1 and t.stride(2) != 1) or (t.shape[1] > 1 and t.stride(1) != t.shape[2]):
        t = t.contiguous()
    return t


def _device_of(*images: Any) -> torch.device:
    for im in images:
        if isinstance(im, torch.Tensor) and im.is_cuda:
            return im.device
    return _device()


def resolve_radius(radius: Any, images: Any) -> float:
    """The image circle's radius for ``params()``: the magnitude of ``get_radius_smart(radius, images)``.  ``"auto"`` on an image
    circle on black is NEGATIVE (the sign quirk of the reference's ``get_radius``, kept on purpose: in a map it means the 180-degree
    flip); the qualifying disc is symmetric about the centre, so only the magnitude matters here, and ``v1c_feat_detect`` takes a positive
    radius only.  An image without a black border raises ``IndexError`` under ``"auto"``, as in ``match_lr``."""
    return abs(float(get_radius_smart(radius, images)))


def _detect_enqueue(t: torch.Tensor, p: FeatParams) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    dev = t.device
    kp = torch.empty((p.max_keypoints, len(KP_FIELDS)), dtype=torch.int32, device=dev)
    desc = torch.empty((p.max_keypoints, 32), dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _native.lib().v1c_feat_detect(dev.index, _stream_ptr(dev), t.data_ptr(), t.shape[0], t.shape[1], t.stride(0), t.shape[2],
                                       C.byref(p), kp.data_ptr(), desc.data_ptr(), count.data_ptr())
    _native.check(rc, "v1c_feat_detect")
    return kp, desc, count


def _match_enqueue(d1: torch.Tensor, d2: torch.Tensor, p: FeatParams) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    dev = d1.device
    n1, n2 = int(d1.shape[0]), int(d2.shape[0])
    cap = max(1, min(n1, n2))
    pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    dist = torch.empty(cap, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _native.lib().v1c_feat_match(dev.index, _stream_ptr(dev), d1.data_ptr() if n1 else None, n1, d2.data_ptr() if n2 else None, n2,
                                      C.byref(p), pairs.data_ptr(), dist.data_ptr(), count.data_ptr())
    _native.check(rc, "v1c_feat_match")
    return pairs, dist, count


def _to_host(*tensors: torch.Tensor) -> list[np.ndarray]:
    """Device tensors -> host arrays with ONE device-to-host copy (one synchronisation): their bytes travel packed."""
    flat = torch.cat([t.contiguous().view(torch.uint8).reshape(-1) for t in tensors]).cpu().numpy()
    out, o = [], 0
    for t in tensors:
        nb = t.numel() * t.element_size()
        out.append(flat[o:o + nb].view(torch.empty((), dtype=t.dtype).numpy().dtype).reshape(tuple(t.shape)))
        o += nb
    return out


def detect(image: Any, *, radius: Any, scale: float = 1.0, **overrides: Any) -> tuple[np.ndarray, np.ndarray]:
    """Keypoints and descriptors of one uint8 image: an ``(N, 6)`` int32 array (columns ``KP_FIELDS``, cell-major) and an ``(N, 32)``
    uint8 array.  ``radius``: the image circle's radius in original pixels, or ``"auto"`` / ``"max"`` (``resolve_radius``: the magnitude of
    what ``get_radius_smart`` gives)."""
    dev = _device_of(image)
    t = _image_tensor(image, dev)
    p = params(scale, resolve_radius(radius, [t]), **overrides)
    kp, desc, count = _to_host(*_detect_enqueue(t, p))
    n = int(count[0])
    return kp[:n].copy(), desc[:n].copy()


def _descriptor_tensor(d: Any, dev: torch.device) -> torch.Tensor:
    t = d if isinstance(d, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(d, dtype=np.uint8)))
    if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != 32:
        raise ValueError(f"descriptors must be an (N, 32) uint8 array, not {tuple(t.shape)} {t.dtype}")
    return t.to(dev).contiguous()


def match(desc1: Any, desc2: Any, **overrides: Any) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Mutual-best Hamming matches of two ``(N, 32)`` uint8 descriptor sets with the ratio test: ``(idx1, idx2, dist)`` in the order of
    ``desc1`` (``max_distance`` [64], ``ratio`` [(3, 4)])."""
    dev = _device_of(desc1, desc2)
    d1, d2 = _descriptor_tensor(desc1, dev), _descriptor_tensor(desc2, dev)
    pairs, dist, count = _to_host(*_match_enqueue(d1, d2, params(**overrides)))
    n = int(count[0])
    return pairs[:n, 0].copy(), pairs[:n, 1].copy(), dist[:n].copy()


def match_points_device(image1: Any, image2: Any, *, scale: float = 1, radius: Any = "auto"):
    """``calibration_cv.match_points`` on the device: ``(points1, points2, kp1, kp2, matches, image1, image2)`` with the points in
    ORIGINAL pixels (the centre of each keypoint's source block), ``kp1`` / ``kp2`` the keypoint arrays of ``detect``, ``matches`` an
    ``(M, 3)`` int32 array of (index into kp1, index into kp2, Hamming distance) and the images as given.  Both eyes share one radius:
    ``resolve_radius(radius, [image1, image2])``, the magnitude of what ``match_lr`` resolves from the same arguments.  Fewer than 3
    matches raise ``ValueError``.

    Two synchronisations: the keypoint counts size the match call (``v1c_feat_match`` takes host counts, so that its grid and scratch
    fit the sets), and one copy at the end brings keypoints, pairs, distances and the match count back together."""
    dev = _device_of(image1, image2)
    t1, t2 = _image_tensor(image1, dev), _image_tensor(image2, dev)
    p = params(scale, resolve_radius(radius, [t1, t2]))
    kp1, desc1, c1 = _detect_enqueue(t1, p)
    kp2, desc2, c2 = _detect_enqueue(t2, p)
    n1, n2 = (int(v) for v in torch.cat([c1, c2]).cpu())
    pairs, dist, count = _match_enqueue(desc1[:n1], desc2[:n2], p)
    k1, k2, pr, dist, count = _to_host(kp1[:n1], kp2[:n2], pairs, dist, count)
    n = int(count[0])
    if n < 3:
        raise ValueError(f"feature matching found {n} match(es) ({n1} / {n2} keypoints); the rotation fit needs at least 3 -- a black or "
                         "textureless pair?")
    pr = pr[:n]
    points1 = k1[pr[:, 0]][:, 4:6] / 2.0
    points2 = k2[pr[:, 1]][:, 4:6] / 2.0
    matches = np.concatenate([pr, dist[:n, None]], axis=1)
    return points1, points2, k1.copy(), k2.copy(), matches, image1, image2
