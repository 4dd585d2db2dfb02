"""Lens vignetting corrected on the device: a radial gain over the image circle (``v1c_vignette_apply_async`` /
``v1c_vignette_rings_async``; INTEGRATION.md section 14 states the contract, tests/vignette_ref.py restates it).

A fisheye loses one to two stops towards the rim of its image circle, and the equirectangular projection stretches that rim over the
largest share of the output.  The model is lensfun's "pa" falloff, ``V(rho) = 1 + k1 rho^2 + k2 rho^4 + k3 rho^6``, and the correction
multiplies every pixel by ``g(rho) = V(rho) ** (-1 / gamma)``.  The only floating-point step is the host's sampling of ``g`` into a
Q14 table (``gain_tables``); the device rule behind it is integer: an exact squared distance, a fixed-point table position, a linear
interpolation of two entries and a rounded product.

``fit_vignette`` fits the three coefficients per channel from ring statistics of a FLAT-FIELD frame -- a white wall, an overcast sky, a
diffuser over the lens -- gathered on the device.  It is not a blind estimate from a scene: whatever the scene does along the radius
ends up in the coefficients.

``remap_tensors``, ``apply``, ``apply_lr`` and ``apply_lr_tensors`` (remapper.py) take the model as ``vignette=``."""
from __future__ import annotations

import ctypes as C
import threading
from collections import OrderedDict
from typing import Any, Sequence

import numpy as np

from . import _native

CHANNELS = ("b", "g", "r")  # the order of a BGR pixel, and of the tables' rows
BINS = 1024                 # intervals of the device's tables: (3, BINS + 1) uint16
Q14 = 1 << 14
GAIN_MAX = 65535 / Q14      # just under 4x, two stops
SCALE_BITS = 30             # the table position's multiplier is below 2^30
R2_BITS = 34                # the largest squared distance the device rule takes is below 2^34
RINGS_MIN, RINGS_MAX = 16, 1024


class VignetteGeom(C.Structure):
    """``v1c_vignette_geom`` (include/vr180_remap.h)"""

    _fields_ = [("cx", C.c_int32), ("cy", C.c_int32), ("scale", C.c_uint32), ("shift", C.c_int32)]


class VignetteRingParams(C.Structure):
    """``v1c_vignette_ring_params`` (include/vr180_remap.h)"""

    _fields_ = [("cx", C.c_int32), ("cy", C.c_int32), ("r2", C.c_int64), ("rings", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32),
                ("reserved", C.c_int32)]


def _coefs(v: Any, what: str) -> tuple[float, float, float]:
    try:
        out = tuple(float(c) for c in v)
    except (TypeError, ValueError):
        raise ValueError(f"Vignette({what}=...): three numbers (k1, k2, k3)") from None
    if len(out) != 3 or not all(np.isfinite(out)):
        raise ValueError(f"Vignette({what}=...): exactly three finite coefficients (k1, k2, k3), not {v!r}")
    return out


class Vignette:
    """The falloff of one lens.  ``coefs=(k1, k2, k3)`` for all channels, ``red=`` / ``green=`` / ``blue=`` for one channel each (the
    missing ones take ``coefs``).  ``V(rho) = 1 + k1 rho^2 + k2 rho^4 + k3 rho^6`` is lensfun's "pa" form, but ``rho`` is the distance
    from the image circle's centre divided by the circle's RADIUS: 1.0 is the rim, the normalisation ``ChromaticAberration`` uses -- it
    is NOT lensfun's half-diagonal, and lensfun's database coefficients do not carry over unscaled.  The gain is
    ``g(rho) = V(rho) ** (-1 / gamma)``: ``gamma=1.0`` for linear-light data, ``gamma=2.2`` folds a power-law encoding into the table so
    that the device never sees a gamma.  Beyond the rim the gain of the rim is held."""

    __slots__ = ("blue", "green", "red", "gamma", "_curve")

    def __init__(self, coefs: Sequence[float] = (0.0, 0.0, 0.0), gamma: float = 1.0, *, red: Sequence[float] | None = None,
                 green: Sequence[float] | None = None, blue: Sequence[float] | None = None):
        base = _coefs(coefs, "coefs")
        self.blue = base if blue is None else _coefs(blue, "blue")
        self.green = base if green is None else _coefs(green, "green")
        self.red = base if red is None else _coefs(red, "red")
        try:
            self.gamma = float(gamma)
        except (TypeError, ValueError):
            raise ValueError(f"Vignette(gamma=...): a positive number, not {gamma!r}") from None
        if not np.isfinite(self.gamma) or self.gamma <= 0:
            raise ValueError(f"Vignette(gamma=...): a positive number, not {gamma!r}")
        self._curve = None

    @classmethod
    def from_rings(cls, rho2: Sequence[float], gains: Any) -> "Vignette":
        """A measured gain curve taken as it is: ``gains[k]`` (one row, or three in BGR order) at ``rho2[k]`` (increasing, within
        [0, 1]), linear in rho^2 between the samples, the end values held outside them."""
        t = np.asarray(rho2, np.float64).ravel()
        g = np.atleast_2d(np.asarray(gains, np.float64))
        if g.shape[0] == 1:
            g = np.repeat(g, 3, axis=0)
        if t.size < 1 or g.shape != (3, t.size):
            raise ValueError(f"Vignette.from_rings: gains must have one value per rho2 ({t.size}) in one or three rows, not {g.shape}")
        if not (np.isfinite(t).all() and np.isfinite(g).all()) or (np.diff(t) <= 0).any() or (g < 0).any():
            raise ValueError("Vignette.from_rings: finite values, rho2 strictly increasing, gains not negative")
        v = cls()
        v._curve = (t.copy(), g.copy())
        return v

    def coefs(self, channel: str) -> tuple[float, float, float]:
        return {"b": self.blue, "g": self.green, "r": self.red}[channel]

    def falloff(self, rho2: Any) -> np.ndarray:
        """``V`` at ``rho2`` (= rho squared), float64, one row per channel in BGR order"""
        t = np.minimum(np.asarray(rho2, np.float64), 1.0)
        if self._curve is not None:
            with np.errstate(divide="ignore"):
                return 1.0 / self.gain(rho2)
        return np.stack([1.0 + t * (k[0] + t * (k[1] + t * k[2])) for k in (self.blue, self.green, self.red)])

    def gain(self, rho2: Any) -> np.ndarray:
        """``g`` at ``rho2``, float64 and unclamped, one row per channel in BGR order; the rim's value beyond 1"""
        t = np.minimum(np.asarray(rho2, np.float64), 1.0)
        if self._curve is not None:
            return np.stack([np.interp(t, self._curve[0], row) for row in self._curve[1]])
        V = self.falloff(t)
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.where(V > 0, np.power(np.maximum(V, 1e-300), -1.0 / self.gamma), np.inf)
        return g

    def key(self) -> tuple:
        """exact, hashable: equal models share it, any other coefficient does not (floats by their bits)"""
        if self._curve is not None:
            return ("curve", self._curve[0].tobytes(), self._curve[1].tobytes())
        return tuple(c.hex() for k in (self.blue, self.green, self.red) for c in k) + (self.gamma.hex(),)

    def spec(self) -> str:
        """the form ``--vignette`` reads (``parse``)"""
        if self._curve is not None:
            raise ValueError("a Vignette made from_rings has no coefficients to print")
        f = lambda k: ",".join(repr(float(c)) for c in k)  # noqa: E731
        if self.blue == self.green == self.red:
            return f(self.green)
        return ";".join(f"{n}:{f(k)}" for n, k in zip(CHANNELS, (self.blue, self.green, self.red)))

    def __repr__(self) -> str:
        if self._curve is not None:
            return f"Vignette.from_rings(<{self._curve[0].size} samples>)"
        return f"Vignette(blue={self.blue}, green={self.green}, red={self.red}, gamma={self.gamma})"


def parse(text: str, gamma: float = 1.0) -> Vignette:
    """``"k1,k2,k3"`` or ``"b:k1,k2,k3;g:...;r:..."`` -> Vignette (the CLI's ``--vignette``); ValueError with a reason"""
    if not isinstance(text, str) or not text.strip():
        raise ValueError("empty vignette specification")

    def nums(s: str) -> list[float]:
        try:
            return [float(v) for v in s.split(",")]
        except ValueError:
            raise ValueError(f"{s.strip()!r}: coefficients must be numbers separated by commas") from None

    if ":" not in text:
        return Vignette(nums(text), gamma)
    got: dict[str, list[float]] = {}
    for part in text.split(";"):
        if not part.strip():
            continue
        name, sep, vals = part.partition(":")
        name = name.strip().lower()
        if not sep or name not in CHANNELS:
            raise ValueError(f"{part.strip()!r}: expected CHANNEL:k1,k2,k3 with CHANNEL one of b, g, r")
        if name in got:
            raise ValueError(f"channel {name!r} given twice")
        got[name] = nums(vals)
    return Vignette(gamma=gamma, red=got.get("r"), green=got.get("g"), blue=got.get("b"))


def parse_pair(text: str, gamma: float = 1.0) -> "Vignette | tuple[Vignette, Vignette]":
    """``--vignette`` of the pair commands: one specification for both eyes, or ``LEFT|RIGHT``"""
    if "|" in text:
        parts = text.split("|")
        if len(parts) != 2:
            raise ValueError("expected LEFT|RIGHT: one '|' between the two eyes' specifications")
        return parse(parts[0], gamma), parse(parts[1], gamma)
    return parse(text, gamma)


def as_per_unit(vignette: Any, n: int) -> list[Vignette]:
    """``vignette=`` of a call with ``n`` units: one object for all of them, or one per unit (the pair entries' ``(left, right)``)"""
    if isinstance(vignette, Vignette):
        return [vignette] * n
    if isinstance(vignette, (tuple, list)) and len(vignette) == n and all(isinstance(v, Vignette) for v in vignette):
        return list(vignette)
    raise TypeError(f"vignette must be a Vignette or one per image ({n}), not {vignette!r}")


def gain_tables(v: Vignette, rho2_max: float = 1.0, bins: int = BINS) -> np.ndarray:
    """``(3, bins + 1)`` uint16, BGR: ``g`` sampled at ``rho^2 = i rho2_max / bins`` in float64, clamped to ``[0, 65535 / 2^14]`` and
    rounded to Q14.  Beyond ``rho = 1`` the value at ``rho = 1`` is held.  The only floating-point step of the correction."""
    if not isinstance(v, Vignette):
        raise TypeError(f"gain_tables: a Vignette is needed, not {v!r}")
    if not (np.isfinite(rho2_max) and rho2_max > 0) or int(bins) < 1:
        raise ValueError("gain_tables: rho2_max must be positive and finite, bins at least 1")
    t = np.arange(int(bins) + 1, dtype=np.float64) * float(rho2_max) / int(bins)
    g = np.clip(np.nan_to_num(v.gain(t), nan=GAIN_MAX, posinf=GAIN_MAX), 0.0, GAIN_MAX)
    return np.floor(g * Q14 + 0.5).astype(np.uint16)


def _dtype_name(dtype: Any) -> str:
    s = str(dtype)
    return s[6:] if s.startswith("torch.") else np.dtype(dtype).name


def check_dtype(dtype: Any, who: str = "vignette") -> None:
    dt = _dtype_name(dtype)
    if dt not in ("uint8", "uint16"):
        raise TypeError(f"{who}: uint8 and uint16 images only, not {dt}")


def round_center(center: Any, h: int, w: int) -> tuple[int, int]:
    """the integer centre of the device rule: ``(W // 2, H // 2)`` for None -- the remap's own default --, else the nearest pixel"""
    if center is None:
        return w // 2, h // 2
    cx, cy = (float(center[0]), float(center[1]))
    if not (np.isfinite(cx) and np.isfinite(cy)):
        raise ValueError(f"vignette: centre {center!r} is not finite")
    return int(np.floor(cx + 0.5)), int(np.floor(cy + 0.5))


def _check_reach(h: int, w: int, cx: int, cy: int) -> None:
    if not (0 < h <= 32767 and 0 < w <= 32767):
        raise ValueError(f"vignette: image size {w} x {h} is outside 1..32767")
    if not (-w <= cx < 2 * w and -h <= cy < 2 * h):
        raise ValueError(f"vignette: centre ({cx}, {cy}) is more than one frame size outside the {w} x {h} frame")


def table_scale(radius: float, rho2_max: float = 1.0, bins: int = BINS) -> tuple[int, int]:
    """``(scale, shift)`` of the table position ``q = (r2 * scale) >> shift`` (8 fraction bits): the multiplier nearest to
    ``256 bins 2^shift / (radius^2 rho2_max)`` with ``2^29 <= scale < 2^30`` -- its rounding moves ``q`` by less than 2^-29 of
    itself -- and ``0 <= shift <= 62``."""
    r = abs(float(radius))
    if not (np.isfinite(r) and r > 0 and np.isfinite(rho2_max) and rho2_max > 0):
        raise ValueError(f"vignette: radius {radius!r} must be finite and not zero")
    ratio = 256.0 * bins / (r * r * float(rho2_max))
    shift = SCALE_BITS - 1 - int(np.floor(np.log2(ratio)))
    scale = int(np.floor(np.ldexp(ratio, shift) + 0.5))
    if scale >= 1 << SCALE_BITS:
        scale, shift = scale >> 1, shift - 1
    if not 0 <= shift <= 62:
        raise ValueError(f"vignette: radius {radius!r} is outside what the table position's fixed point takes")
    return scale, shift


def geometry(h: int, w: int, center: Any, radius: float, rho2_max: float = 1.0) -> VignetteGeom:
    cx, cy = round_center(center, h, w)
    _check_reach(h, w, cx, cy)
    scale, shift = table_scale(radius, rho2_max)
    return VignetteGeom(cx, cy, scale, shift)


def ring_r2(radius: float) -> int:
    """the ring statistics' squared radius: the nearest integer, at least 1"""
    r = abs(float(radius))
    if not (np.isfinite(r) and r > 0):
        raise ValueError(f"vignette: radius {radius!r} must be finite and not zero")
    r2 = max(1, int(np.floor(r * r + 0.5)))
    if r2 >= 1 << (R2_BITS + 1):
        raise ValueError(f"vignette: radius {radius!r} is too large")
    return r2


def default_mask(dtype: Any) -> tuple[int, int]:
    """``lo``, ``hi`` of the ring statistics: the black (below 4 %) and the clipped (the top code) are left out"""
    return (10, 254) if _dtype_name(dtype) == "uint8" else (2570, 65534)


# ---- the device entries -----------------------------------------------------------------------------------------------------------------
def _image_args(image: Any, who: str):
    import torch

    from .remapper import _check_image_tensor

    if not isinstance(image, torch.Tensor) or not image.is_cuda:
        raise TypeError(f"{who}: a CUDA tensor is needed")
    check_dtype(image.dtype, who)  # (before any launch)
    _check_image_tensor(image, "image")
    h, w, cn = (int(v) for v in image.shape)
    es = image.element_size()
    return h, w, cn, es, (image.stride(0) if h > 1 else w * cn) * es


def tables_tensor(vignette: Vignette, device: Any, rho2_max: float = 1.0):
    """``gain_tables`` uploaded: the ``tables=`` of ``apply_vignette_tensor``, to be kept across the frames of a shoot"""
    import torch

    return torch.from_numpy(gain_tables(vignette, rho2_max)).to(device)


def apply_vignette_tensor(image: Any, vignette: Vignette | None, *, center: Any = None, radius: float, out: Any = None,
                          tables: Any = None):
    """``out = image * g(rho)`` by the integer rule, on the colour channels; a fourth channel is copied, a grey image takes the green
    table.  ``center``: ``(cx, cy)`` in pixels, rounded to the nearest pixel (None: ``(W // 2, H // 2)``); ``radius``: the image
    circle's, in pixels.  ``out=None`` allocates, ``out=image`` rewrites in place.  One launch on the current stream, nothing
    synchronised.  ``tables``: a ``(3, 1025)`` uint16 device tensor (``tables_tensor``) instead of ``vignette``'s own, which costs an
    upload per call.  uint8 and uint16 images; float32 raises TypeError before any launch."""
    import torch

    from .remapper import _stream_ptr

    h, w, cn, es, ps = _image_args(image, "apply_vignette_tensor")
    geom = geometry(h, w, center, radius)
    dev = image.device
    if tables is None:
        tables = tables_tensor(vignette, dev)
    elif not isinstance(tables, torch.Tensor) or tables.dtype not in (torch.uint16, torch.int16) or tables.numel() != 3 * (BINS + 1) \
            or not tables.is_contiguous() or tables.device != dev:
        raise ValueError(f"apply_vignette_tensor: tables must be a contiguous (3, {BINS + 1}) uint16 tensor on the image's device")
    if out is None:
        out = torch.empty((h, w, cn), dtype=image.dtype, device=dev)
    h2, w2, cn2, es2, pd = _image_args(out, "apply_vignette_tensor")
    if (h, w, cn, es) != (h2, w2, cn2, es2) or out.device != dev:
        raise ValueError("apply_vignette_tensor: out must have the image's shape, type and device")
    rc = _native.lib().v1c_vignette_apply_async(dev.index, _stream_ptr(dev), image.data_ptr(), ps, out.data_ptr(), pd, h, w, cn, es,
                                                C.byref(geom), tables.data_ptr())
    _native.check(rc, "v1c_vignette_apply_async")
    return out


def vignette_rings_tensor(image: Any, *, center: Any = None, radius: float, rings: int = 256, lo: int | None = None,
                          hi: int | None = None):
    """The ring statistics of ``image``: a ``(rings, 4)`` int64 tensor ``(sumB, sumG, sumR, n)`` left on the device -- over every pixel
    inside the circle whose colour channels all lie in ``[lo, hi]`` (default: the black and the clipped left out), the rings uniform in
    rho^2 (equal areas).  A grey image fills ``sumG`` only.  Two launches on the current stream, nothing synchronised."""
    import torch

    from .remapper import _stream_ptr

    h, w, cn, es, ps = _image_args(image, "vignette_rings_tensor")
    cx, cy = round_center(center, h, w)
    _check_reach(h, w, cx, cy)
    dlo, dhi = default_mask(image.dtype)
    prm = VignetteRingParams(cx, cy, ring_r2(radius), int(rings), dlo if lo is None else int(lo), dhi if hi is None else int(hi), 0)
    dev = image.device
    out = torch.empty((int(rings) if RINGS_MIN <= int(rings) <= RINGS_MAX else 1, 4), dtype=torch.int64, device=dev)
    rc = _native.lib().v1c_vignette_rings_async(dev.index, _stream_ptr(dev), image.data_ptr(), ps, h, w, cn, es, C.byref(prm),
                                                out.data_ptr())
    _native.check(rc, "v1c_vignette_rings_async")
    return out


def fit_rings(stats: Any, *, gamma: float = 1.0, min_pixels: int = 16, center_rings: int | None = None, grey: bool = False) -> Vignette:
    """The host half of ``fit_vignette``, float64: ``stats`` is the ``(rings, 4)`` record ``(sumB, sumG, sumR, n)``.  Per channel, a
    count-weighted least squares of ``(mean(rho) / mean(0)) ** gamma - 1`` on ``(rho^2, rho^4, rho^6)``, ``rho^2`` at each ring's area
    midpoint ``(k + 1/2) / rings``; rings with fewer than ``min_pixels`` are left out; ``mean(0)`` is the mean over the innermost
    ``center_rings`` populated rings (default ``rings // 64``, at least 1), divided by the fitted falloff at those rings in three
    further passes -- they sit a little way down the curve themselves.  ValueError where too few rings are populated."""
    s = np.asarray(stats, np.int64)
    if s.ndim != 2 or s.shape[1] != 4:
        raise ValueError(f"fit_rings: a (rings, 4) record is needed, not {s.shape}")
    rings = s.shape[0]
    n = s[:, 3].astype(np.float64)
    keep = np.flatnonzero(s[:, 3] >= max(1, int(min_pixels)))
    if keep.size < 4:
        raise ValueError(f"fit_vignette: {keep.size} of {rings} rings hold {max(1, int(min_pixels))} pixels or more inside the mask; "
                         "at least 4 are needed (is the frame a flat field, and are lo / hi right for it?)")
    t = (keep + 0.5) / rings
    inner = keep[: max(1, rings // 64 if center_rings is None else int(center_rings))]
    A = np.stack([t, t * t, t * t * t], axis=1) * np.sqrt(n[keep])[:, None]
    coefs = []
    for c in ((1, 1, 1) if grey else (0, 1, 2)):
        m0 = s[inner, c].sum() / n[inner].sum()
        if m0 <= 0:
            raise ValueError("fit_vignette: the centre of the frame is black inside the mask")
        ti = float(((inner + 0.5) / rings * n[inner]).sum() / n[inner].sum())
        k = np.zeros(3)
        for _ in range(4):
            at_inner = 1.0 + ti * (k[0] + ti * (k[1] + ti * k[2]))  # (V where mean(0) was taken, by the fit so far)
            y = np.power(s[keep, c] / n[keep] / m0, float(gamma)) * at_inner - 1.0
            k, *_ = np.linalg.lstsq(A, y * np.sqrt(n[keep]), rcond=None)
        coefs.append(tuple(float(v) for v in k))
    return Vignette(gamma=gamma, blue=coefs[0], green=coefs[1], red=coefs[2])


def fit_vignette(image: Any, *, center: Any = None, radius: Any, rings: int = 256, lo: int | None = None, hi: int | None = None,
                 gamma: float = 1.0, min_pixels: int = 16, center_rings: int | None = None, device: Any = None) -> Vignette:
    """The ``Vignette`` of a flat-field frame: a white wall, an overcast sky, or a diffuser over the lens -- NOT a blind estimate from
    a scene.  The ring statistics are gathered on the device (``vignette_rings_tensor``) and brought to the host with one
    synchronisation; the fit is ``fit_rings``.  ``center``: ``(cx, cy)``, None or ``"auto"``; ``radius``: pixels or ``"fit"`` (both
    from ``circle.fit_circle``).  ``gamma``: the encoding of the frame (1.0: linear light); it becomes the result's ``gamma``.
    ValueError where the mask leaves too little."""
    import torch

    from . import remapper

    if not isinstance(image, torch.Tensor):
        check_dtype(np.asarray(image).dtype, "fit_vignette")
        image = remapper._to_device(image, remapper._device(device))
    check_dtype(image.dtype, "fit_vignette")
    if isinstance(center, str) or isinstance(radius, str):
        from . import circle

        if (isinstance(center, str) and center != "auto") or (isinstance(radius, str) and radius != "fit"):
            raise ValueError('fit_vignette: center is (cx, cy), None or "auto"; radius is a number or "fit"')
        f = circle.fit_circle(image)
        center = (f.cx, f.cy) if isinstance(center, str) else center
        radius = f.radius if isinstance(radius, str) else radius
    stats = vignette_rings_tensor(image, center=center, radius=radius, rings=rings, lo=lo, hi=hi).cpu().numpy()
    return fit_rings(stats, gamma=gamma, min_pixels=min_pixels, center_rings=center_rings, grey=int(image.shape[2]) == 1)


_TABLES: "OrderedDict[tuple, Any]" = OrderedDict()  # the models' tables on the device, least recently used last out
_TABLES_MAX = 16
_TABLES_LOCK = threading.Lock()


def cached_tables(vignette: Vignette, device: Any):
    """``tables_tensor`` kept per model and device: the frames of a shoot share one upload, and a call repeated under graph capture
    uploads nothing"""
    key = (vignette.key(), str(device))
    with _TABLES_LOCK:
        t = _TABLES.get(key)
        if t is not None:
            _TABLES.move_to_end(key)
            return t
    t = tables_tensor(vignette, device)
    with _TABLES_LOCK:
        _TABLES[key] = t
        while len(_TABLES) > _TABLES_MAX:
            _TABLES.popitem(last=False)
    return t


def correct_sources(srcs: Sequence[Any], vignette: Any, *, centers: Sequence[Any] | None, radius: float, inplace: Any = False) -> list:
    """``vignette=`` of the remap entries: every source corrected into a temporary (``inplace``, one flag or one per source: where it
    lies -- tensors the call uploaded or decoded itself), with the centre and radius the remap uses.  One launch per source on the
    current stream."""
    vs = as_per_unit(vignette, len(srcs))
    for s in srcs:
        check_dtype(s.dtype)
    flags = [bool(inplace)] * len(srcs) if isinstance(inplace, bool) else [bool(f) for f in inplace]
    return [apply_vignette_tensor(s, v, center=None if centers is None else centers[k], radius=radius, out=s if flags[k] else None,
                                  tables=cached_tables(v, s.device)) for k, (s, v) in enumerate(zip(srcs, vs))]
