"""``get_map`` / ``apply`` / ``apply_lr`` of the reference, running on MI355X.

Drop-in for ``vr180_convert/remapper.py`` (same names, keyword signatures incl. the ``boarder_*``
spelling, return types and error behaviour).  Instead of evaluating the transformer chain as
NumPy passes over a meshgrid and handing a float32 map to ``cv2.remap`` (remapper.py:50-58,
388-398), the chain is lowered once (``chain.lower_for_get_map``) and evaluated per output pixel
inside the HIP kernel that also does cv2.remap's fixed-point gather; eyes are written straight
into their half of the side-by-side buffer (remapper.py:517-518).

Inputs may be paths, ``numpy`` arrays (uploaded, results come back as ``numpy``) or CUDA
``torch`` tensors (device-resident in and out -- what ``bench.py`` times).
"""
from __future__ import annotations

import ctypes as C
import threading
import time
from collections import OrderedDict
import logging
from logging import getLogger
from pathlib import Path
from typing import Any, Literal, Sequence

import numpy as np
import torch
from numpy.typing import NDArray

from . import _abi, _hostpipe, _io, _native
from .chain import NotLowerable, TransformerBase, denormalize_center, get_radius, lower_for_get_map
from .chain import DenormalizeTransformer, NormalizeTransformer

LOG = getLogger(__name__)

INTER_LANCZOS4 = _abi.INTER_LANCZOS4
BORDER_CONSTANT = _abi.BORDER_CONSTANT


# --------------------------------------------------------------------------------------------
# device plumbing
# --------------------------------------------------------------------------------------------
def _device(device: Any = None) -> torch.device:
    if not torch.cuda.is_available():
        raise _native.EngineUnavailable(
            "no HIP device visible: vr180_convert_amd runs the remap on an MI355X and has no CPU fallback"
        )
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    d = torch.device(device)
    if d.type != "cuda":
        raise ValueError("device must be a cuda (HIP) device")
    return torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())


try:  # the raw handle of the current stream without building a torch.cuda.Stream object (4 us per call)
    _raw_stream = torch._C._cuda_getCurrentRawStream
except AttributeError:  # pragma: no cover
    _raw_stream = None


def _stream_ptr(dev: torch.device) -> int:
    if _raw_stream is not None and dev.index is not None:
        return int(_raw_stream(dev.index))
    return int(torch.cuda.current_stream(dev).cuda_stream)


def border_scalar(value: Any) -> np.ndarray:
    """Python ``borderValue`` -> saturated uint8[4] the way cv2 fills its Scalar: a bare int sets
    only component 0, a tuple sets the leading components."""
    vals = [value] if np.isscalar(value) else list(value)
    out = np.zeros(4, np.uint8)
    for i, v in enumerate(vals[:4]):
        out[i] = int(min(255, max(0, np.rint(float(v)))))
    return out


def border_scalar_f64(value: Any) -> np.ndarray:
    """Python ``borderValue`` -> the float64[4] cv2 Scalar itself (a bare number sets only component 0, a tuple the leading
    components): what ``v1c_plan_create_ex`` saturates to the pixel type of a 16-bit or float32 image."""
    vals = [value] if np.isscalar(value) else list(value)
    out = np.zeros(4, np.float64)
    for i, v in enumerate(vals[:4]):
        out[i] = float(v)
    return out


# pixel types cv2.remap takes (CV_8U, CV_16U, CV_32F) -> the engine's depth codes; anything else raises TypeError
DEPTHS = {torch.uint8: _abi.DEPTH_8U, torch.uint16: _abi.DEPTH_16U, torch.float32: _abi.DEPTH_32F}
NP_DTYPES = (np.uint8, np.uint16, np.float32)


def _border_key(value: Any, dtype: torch.dtype) -> bytes:
    """The part of a cache key the border colour decides: the saturated uint8 colour for 8-bit images (as ever), the Scalar otherwise."""
    return border_scalar(value).tobytes() if dtype == torch.uint8 else border_scalar_f64(value).tobytes()


def _check_image_tensor(t: torch.Tensor, what: str) -> None:
    if t.dtype not in DEPTHS or t.dim() != 3:
        raise TypeError(f"{what} must be a uint8, uint16 or float32 (H, W, C) tensor")
    cn = t.shape[2]
    if (cn > 1 and t.stride(2) != 1) or (t.shape[1] > 1 and t.stride(1) != cn) or (
        t.shape[0] > 1 and t.stride(0) < t.shape[1] * cn
    ):
        raise ValueError(f"{what}: pixels must be contiguous within a row (column-sliced views are fine)")


def marshal_units(srcs: Sequence[torch.Tensor], dsts: Sequence[torch.Tensor], rots: Sequence[Any] | None, *,
                  src_hw: tuple[int, int], dst_wh: tuple[int, int], cn: int, device: torch.device | None,
                  dtype: torch.dtype | None = None):
    """The ``v1c_unit`` array of a launch (include/vr180_remap.h): one record per eye -- pointers and row
    pitches of its source view and of ITS half of the side-by-side output (remapper.py:517-518 becomes a
    pitch, in bytes), optionally the 3x3 rotation replacing the chain's.  Validates shapes, layout, pixel type and device;
    ``device=None`` skips the device check (the multi-rank CPU tests marshal host tensors)."""
    n = len(srcs)
    units = (_abi.Unit * n)()
    for k, (s, d) in enumerate(zip(srcs, dsts)):
        _check_image_tensor(s, "src")
        _check_image_tensor(d, "dst")
        if s.dtype != d.dtype or (dtype is not None and s.dtype != dtype):
            raise TypeError(f"unit {k}: src {s.dtype} / dst {d.dtype}: source and destination must both have the plan's pixel type"
                            + ("" if dtype is None else f" ({dtype})"))
        if tuple(s.shape) != (*src_hw, cn) or tuple(d.shape) != (dst_wh[1], dst_wh[0], cn):
            raise ValueError(f"unit {k}: tensor shapes {tuple(s.shape)} -> {tuple(d.shape)} do not match the plan")
        if device is not None and (s.device != device or d.device != device):
            raise ValueError(f"unit {k}: tensors must live on {device}")
        units[k].src, units[k].dst = s.data_ptr(), d.data_ptr()
        units[k].src_pitch, units[k].dst_pitch = s.stride(0) * s.element_size(), d.stride(0) * d.element_size()
        if rots is not None and rots[k] is not None:
            m = np.asarray(rots[k], dtype=np.float64).reshape(9)
            units[k].has_rot = 1
            for q in range(9):
                units[k].rot[q] = m[q]
    return units


class Plan:
    """Owner of one ``v1c_plan`` (see include/vr180_remap.h: v1c_plan_create)."""

    def __init__(self, chain: _abi.Chain, *, src_hw, dst_wh, cn, interpolation, border_mode, border_value, device,
                 dtype: torch.dtype = torch.uint8):
        self.device = _device(device)
        self.src_hw, self.dst_wh, self.cn = tuple(src_hw), tuple(dst_wh), int(cn)
        if dtype not in DEPTHS:
            raise TypeError(f"pixel type {dtype}: uint8, uint16 or float32 only (cv2.remap's CV_8U / CV_16U / CV_32F)")
        self.dtype = dtype
        self._h = C.c_void_p()
        self._memo: "OrderedDict[tuple, Any]" = OrderedDict()  # marshalled unit arrays of recent buffer sets
        t0 = time.perf_counter()
        if dtype == torch.uint8:
            bv = border_scalar(border_value)
            rc = _native.lib().v1c_plan_create(
                C.byref(self._h), self.device.index, C.byref(chain), src_hw[0], src_hw[1], dst_wh[1], dst_wh[0],
                cn, int(interpolation), int(border_mode), bv.ctypes.data,
            )
            _native.check(rc, "v1c_plan_create")
        else:  # 16-bit / float32 (k_remap_wide): the border colour travels as cv2's Scalar of doubles
            bv = border_scalar_f64(border_value)
            rc = _native.lib().v1c_plan_create_ex(
                C.byref(self._h), self.device.index, C.byref(chain), src_hw[0], src_hw[1], dst_wh[1], dst_wh[0],
                cn, DEPTHS[dtype], int(interpolation), int(border_mode), bv.ctypes.data,
            )
            _native.check(rc, "v1c_plan_create_ex")
        self.create_ms = (time.perf_counter() - t0) * 1e3  # synchronous: host analysis + table uploads + tile boxes

    @property
    def path(self) -> str:
        """'ray' (fused separable tables + radial table), 'planar' (the same kernels on the normalised plane point: chains that do not start
        with an EquirectangularEncoder) or 'literal' (fp64 interpreter)."""
        return {1: "ray", 2: "planar"}.get(_native.lib().v1c_plan_path(self._h), "literal")

    def last_launch(self) -> str:
        """Kernel family of this plan's most recent launch group (``v1c_plan_last_launch``): 'generic', 'tile', 'mirror', 'batch',
        'rot_pair', 'cn', 'cn_rot' or 'wide' (16-bit / float32 images), with '+fixup' when a fix-up pass followed; '' before the first
        run.  For tests and the bench."""
        k = _native.lib().v1c_plan_last_launch(self._h)
        if k < 0:
            return ""
        return _abi.LAUNCH_NAMES.get(k & 0xFF, "?") + ("+fixup" if k & _abi.LAUNCH_FIXUP else "")

    def tap_table_bytes(self) -> int:
        """Bytes of the plan's tap table (``v1c_plan_tap_table_bytes``): the per-lane tap coordinates a rest-free pair plan keeps so
        that its launches need not evaluate the map; 0 when the plan holds none (or the library behind ``V1C_LIB`` predates it)."""
        f = getattr(_native.lib(), "v1c_plan_tap_table_bytes", None)
        return int(f(self._h)) if f is not None else 0

    def tap_entry_bytes(self) -> int:
        """Bytes per lane of that table (``v1c_plan_tap_entry_bytes``): 12, or 8 for the compact entry that plans with large tables
        keep; 0 when the plan holds none.  A library behind ``V1C_LIB`` that predates the compact entry holds 12-byte entries."""
        f = getattr(_native.lib(), "v1c_plan_tap_entry_bytes", None)
        if f is None:
            return 12 if self.tap_table_bytes() else 0
        return int(f(self._h))

    def run(self, srcs: Sequence[torch.Tensor], dsts: Sequence[torch.Tensor], rots: Sequence[Any] | None = None) -> None:
        n = len(srcs)
        if n == 0 or len(dsts) != n or (rots is not None and len(rots) != n):
            raise ValueError("srcs / dsts / rots lengths differ or are empty")
        # a steady stream of calls on the same buffers (video frames written in place, bench steps):
        # the validated, marshalled unit array of the previous call is reused
        sig = None
        if rots is None:
            try:
                sig = tuple((s.data_ptr(), s.stride(), s.shape, s.dtype, d.data_ptr(), d.stride(), d.shape, d.dtype) for s, d in zip(srcs, dsts))
            except AttributeError:
                sig = None
            # (a few buffer sets are remembered: double / triple buffering rotates them; dict get / set of one key
            # are atomic under the GIL, an entry is written once and never mutated)
            units = self._memo.get(sig) if sig is not None else None
            if units is not None:
                rc = _native.lib().v1c_plan_run(self._h, _stream_ptr(self.device), units, n)
                _native.check(rc, "v1c_plan_run")
                return
        units = marshal_units(srcs, dsts, rots, src_hw=self.src_hw, dst_wh=self.dst_wh, cn=self.cn, device=self.device, dtype=self.dtype)
        rc = _native.lib().v1c_plan_run(self._h, _stream_ptr(self.device), units, n)
        _native.check(rc, "v1c_plan_run")
        if sig is not None:
            self._memo[sig] = units
            while len(self._memo) > 64:
                try:
                    self._memo.popitem(last=False)
                except KeyError:  # another thread emptied it
                    break

    def run_auto(self, srcs: Sequence[torch.Tensor], dsts: Sequence[torch.Tensor], rad: torch.Tensor | None = None,
                 rots: Sequence[Any] | None = None, threshold: int = 10) -> None:
        """``v1c_plan_run_auto``: the launch with the radius read from device memory -- ``rad`` = float64 ``(n, 2)`` (radius, status)
        pairs as ``v1c_get_radius_async`` writes them; the launch uses their maximum.  ``rad=None``: the estimates are taken from
        ``srcs`` themselves by the same call (``v1c_plan_run_auto_images``, ``threshold`` = get_radius's).  Raises NotImplementedError
        for chains / geometries / pixel types the device-resident form does not serve (the caller then takes the radius to the host)."""
        units = marshal_units(srcs, dsts, rots, src_hw=self.src_hw, dst_wh=self.dst_wh, cn=self.cn, device=self.device, dtype=self.dtype)
        if rad is None:
            rc = _native.lib().v1c_plan_run_auto_images(self._h, _stream_ptr(self.device), units, len(srcs), int(threshold))
            _native.check(rc, "v1c_plan_run_auto_images")
            return
        if rad.dtype != torch.float64 or rad.dim() != 2 or rad.shape[1] != 2 or not rad.is_contiguous() or rad.device != self.device:
            raise ValueError("rad must be a contiguous float64 (n, 2) tensor on the plan's device")
        rc = _native.lib().v1c_plan_run_auto(self._h, _stream_ptr(self.device), units, len(srcs), rad.data_ptr(), int(rad.shape[0]))
        _native.check(rc, "v1c_plan_run_auto")

    def run_units(self, units: Any, n: int) -> None:
        """Launch an already marshalled ``v1c_unit`` array (``marshal_units``) on the current stream."""
        rc = _native.lib().v1c_plan_run(self._h, _stream_ptr(self.device), units, int(n))
        _native.check(rc, "v1c_plan_run")

    def release_captures(self) -> None:
        """Hand the plan's capture-owned unit buffers out again (``v1c_plan_release_captures``): a graph-captured launch of more than
        16 units keeps one of 4; call this once the graphs that recorded them are destroyed."""
        _native.check(_native.lib().v1c_plan_release_captures(self._h), "v1c_plan_release_captures")

    def get_map(self, rot: Any = None) -> tuple[torch.Tensor, torch.Tensor]:
        w, h = self.dst_wh
        xm = torch.empty((h, w), dtype=torch.float32, device=self.device)
        ym = torch.empty((h, w), dtype=torch.float32, device=self.device)
        r = None if rot is None else np.ascontiguousarray(np.asarray(rot, np.float64).reshape(9))
        rc = _native.lib().v1c_plan_get_map(
            self._h, _stream_ptr(self.device), xm.data_ptr(), ym.data_ptr(), xm.stride(0) * 4,
            None if r is None else r.ctypes.data,
        )
        _native.check(rc, "v1c_plan_get_map")
        return xm, ym

    def __del__(self):
        try:
            if self._h:
                _native.lib().v1c_plan_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass


_PLANS: "OrderedDict[tuple, Plan]" = OrderedDict()
_PLAN_CACHE_SIZE = 32
_PLANS_LOCK = threading.Lock()  # one worker thread per device (sharding.py) shares this cache


_AUTO_LAST: dict = {}  # (chain, geometry) -> the radius its last radius="auto" call found on the host (_remap_host_radius)
_TLS = threading.local()  # .plans: the plans the calling thread's last remap_tensors ran (last_launch_kinds)


class _LutLaunch:
    """A unit remapped from a host-computed map (``v1c_remap_lut``: chains that cannot be lowered), as ``last_launch_kinds`` reports it."""

    @staticmethod
    def last_launch() -> str:
        return "lut"


def last_launch_kinds() -> list[str]:
    """Kernel family per launch group of the calling thread's most recent ``remap_tensors`` / ``apply_lr_tensors`` call
    (``Plan.last_launch``: 'generic', 'tile', 'mirror', 'batch', 'rot_pair', 'cn', 'cn_rot', '+fixup' appended when a fix-up pass followed;
    'lut' per unit whose map came from the chain's own ``transform()``).  The engine serves the same bytes through several kernels; tests
    use this to make sure a case meant for a tiled kernel reached it."""
    return [p.last_launch() for p in getattr(_TLS, "plans", [])]


def last_tap_table_bytes() -> list[int]:
    """``Plan.tap_table_bytes`` per launch group of the calling thread's most recent ``remap_tensors`` / ``apply_lr_tensors`` call, in
    the order of ``last_launch_kinds`` (0: that plan evaluates its map in every launch; units served from a host map count 0)."""
    return [p.tap_table_bytes() if isinstance(p, Plan) else 0 for p in getattr(_TLS, "plans", [])]


def last_tap_entry_bytes() -> list[int]:
    """``Plan.tap_entry_bytes`` per launch group, in the order of ``last_tap_table_bytes`` (0: no table)."""
    return [p.tap_entry_bytes() if isinstance(p, Plan) else 0 for p in getattr(_TLS, "plans", [])]


def last_auto_radius_form() -> str:
    """Which form the calling thread's most recent ``apply_lr_tensors(radius="auto")`` (or successful ``remap_tensors_auto``) took: 'device'
    (``remap_tensors_auto``: the radius never left the GPU) or 'exact' (estimates brought to the host); '' before the first such call.
    For tests and the bench."""
    return getattr(_TLS, "auto_form", "")


def clear_caches() -> None:
    """Forget every plan and lowered chain (cold-call measurements, tests)."""
    with _PLANS_LOCK:
        _PLANS.clear()
        _LOWERED.clear()
        _LAST_SHARED[0] = None
        _AUTO_LAST.clear()
    import sys

    ca = sys.modules.get(__package__ + ".chromatic")  # (its plans too, when the module was ever used)
    if ca is not None:
        ca.clear_caches()
    vg = sys.modules.get(__package__ + ".vignette")  # (and its tables on the device)
    if vg is not None:
        vg._TABLES.clear()


def _plan_for(chain: _abi.Chain, *, src_hw, dst_wh, cn, interpolation, border_mode, border_value, device,
              dtype: torch.dtype = torch.uint8) -> Plan:
    dev = _device(device)
    key = (chain.key(), tuple(src_hw), tuple(dst_wh), cn, int(interpolation), int(border_mode),
           _border_key(border_value, dtype), dev.index, dtype)
    with _PLANS_LOCK:
        plan = _PLANS.get(key)
        if plan is not None:
            _PLANS.move_to_end(key)
            return plan
    # created outside the lock (tens of ms: other devices' threads keep going); a racing duplicate is dropped
    plan = Plan(chain, src_hw=src_hw, dst_wh=dst_wh, cn=cn, interpolation=interpolation,
                border_mode=border_mode, border_value=border_value, device=dev, dtype=dtype)
    with _PLANS_LOCK:
        plan = _PLANS.setdefault(key, plan)
        _PLANS.move_to_end(key)
        while len(_PLANS) > _PLAN_CACHE_SIZE:
            _PLANS.popitem(last=False)
    return plan


def _split_single_rotation(chain: _abi.Chain) -> tuple[_abi.Chain, np.ndarray | None]:
    """Chains that differ only in the matrix of their single rotate stage (BASELINE config 5:
    per-frame, per-eye calibration, cli.py:308-319) share one plan: returns the chain with that
    matrix blanked plus the matrix, which then travels per unit (v1c_unit.rot).  Chains with no
    or several rotate stages are returned unchanged."""
    idx = [i for i in range(chain.n_ops) if chain.ops[i].opcode == _abi.OP_ROTATE]
    if len(idx) != 1:
        return chain, None
    i = idx[0]
    rot = np.array(chain.ops[i].p[:9], dtype=np.float64)
    blank = _abi.Chain.from_buffer_copy(bytes(chain))
    for q in range(9):
        blank.ops[i].p[q] = 1.0 if q in (0, 4, 8) else 0.0
    return blank, rot


def _host_map(transformer: TransformerBase, *, radius, size_input, size_output, center=None):
    """The reference's own recipe (remapper.py:50-58) for chains that cannot be lowered: user
    subclasses only expose NumPy ``transform``, so the map has to be computed by calling it.
    ``center`` = (cx, cy): the image circle's centre instead of ``(W_in // 2, H_in // 2)``."""
    xmap, ymap = np.meshgrid(np.arange(size_output[0]), np.arange(size_output[1]))
    full = (
        NormalizeTransformer()
        * transformer
        * DenormalizeTransformer(scale=(radius, radius), center=denormalize_center(size_input, center))
    )
    xmap, ymap = full.transform(xmap, ymap)
    return xmap.astype(np.float32), ymap.astype(np.float32)


_LOWERED: "OrderedDict[tuple, _abi.Chain]" = OrderedDict()
_LAST_SHARED: list = [None]  # [(key, Plan)] of the last remap_tensors call with one shared transformer


class _NoKey(Exception):
    """The transformer holds state the memo key cannot capture exactly: lower it on every call."""


_FIELD_NAMES: dict = {}  # type -> tuple of dataclass field names (built-in stages), None (a foreign dataclass), False (no dataclass)


def _param_key(obj: Any):
    """Exact, hashable image of a built-in transformer's parameters: floats by their bits
    (``float.hex``), arrays by dtype / shape / bytes, quaternion-likes by their four components,
    dataclass stages field by field.  ``repr`` is NOT used: NumPy prints arrays with 8 digits and
    honours ``np.set_printoptions``, numpy-quaternion prints ``%.15g`` -- two rotations 2e-9
    apart would share a key and the second call would silently reuse the first one's plan.
    (Runs on every call of the device-resident API: exact-type tests first, field names cached per class.)"""
    t = type(obj)
    if t is float:
        return ("f", obj.hex())
    if t is int:
        return ("i", obj)
    if obj is None or t is bool or t is str or t is bytes:
        return obj
    names = _FIELD_NAMES.get(t, 0)
    if names == 0:
        import dataclasses

        if dataclasses.is_dataclass(t):
            # a user subclass may carry state outside its fields
            names = tuple(f.name for f in dataclasses.fields(t)) if t.__module__ == TransformerBase.__module__ else None
        else:
            names = False
        _FIELD_NAMES[t] = names
    if names is None:
        raise _NoKey
    if names is not False:
        return (t.__name__, tuple([_param_key(getattr(obj, n)) for n in names]))
    if isinstance(obj, (bool, str, bytes)):
        return obj
    if isinstance(obj, (int, np.integer)):
        return ("i", int(obj))
    if isinstance(obj, (float, np.floating)):
        return ("f", float(obj).hex())
    if isinstance(obj, np.ndarray):
        if obj.dtype == object:
            raise _NoKey
        a = np.ascontiguousarray(obj)
        return ("nd", a.dtype.str, a.shape, a.tobytes())
    if isinstance(obj, (list, tuple)):
        return (t.__name__, tuple([_param_key(v) for v in obj]))
    if all(hasattr(obj, c) for c in "wxyz"):
        return ("q", tuple(float(getattr(obj, c)).hex() for c in "wxyz"))
    raise _NoKey


def _transformer_key(t: Any):
    try:
        return _param_key(t)
    except (_NoKey, TypeError, ValueError):
        return None


def _lower_cached(t: TransformerBase, *, radius, size_input, size_output, center=None) -> _abi.Chain:
    """``lower_for_get_map`` memoised on the chain's exact parameter set (``_param_key``): a steady
    stream of identical calls -- frames of a video, bench steps -- lowers once.  Chains holding
    anything the key cannot capture exactly (user subclasses, object arrays) are lowered every time.
    An explicit ``center`` joins the key by its bits; ``None`` leaves the key what it has always been."""
    k = _transformer_key(t)
    if k is None:
        return lower_for_get_map(t, radius=radius, size_input=size_input, size_output=size_output, center=center)
    key = (k, float(radius).hex(), tuple(size_input), tuple(size_output))
    if center is not None:
        key += (("center", float(center[0]).hex(), float(center[1]).hex()),)
    with _PLANS_LOCK:  # (the per-device worker threads of sharding.remap_sharded share this cache)
        ch = _LOWERED.get(key)
    if ch is None:
        ch = lower_for_get_map(t, radius=radius, size_input=size_input, size_output=size_output, center=center)
        with _PLANS_LOCK:
            _LOWERED[key] = ch
            while len(_LOWERED) > 64:
                _LOWERED.popitem(last=False)
    return ch


def remap_tensors(
    transformer: TransformerBase | Sequence[TransformerBase],
    srcs: Sequence[torch.Tensor],
    dsts: Sequence[torch.Tensor],
    *,
    radius: float,
    interpolation: int = INTER_LANCZOS4,
    boarder_mode: int = BORDER_CONSTANT,
    boarder_value: Any = 0,
    size_input: tuple[int, int] | None = None,
    rotations: Sequence[Any] | None = None,
    center: Any = None,
    chromatic: Any = None,
    vignette: Any = None,
) -> list[str]:
    """Device-resident core of ``apply``: remap every ``srcs[k]`` into ``dsts[k]`` (same device,
    same shapes) on the current stream.  ``transformer`` is one chain shared by all units
    (remapper.py:381-398) or one per unit.  ``rotations`` (optional, one 3x3 matrix or quaternion
    per unit) replaces the rotation of the chain's single ``Euclidean3DRotator`` per unit -- the
    per-frame, per-eye calibration of the CLI (cli.py:308-319) without lowering a chain per unit.
    ``center``: the image circle's centre in source pixels instead of ``(W_in // 2, H_in // 2)`` -- one ``(cx, cy)`` for every unit,
    one per unit (``None`` entries keep the frame's), or ``"auto"``: fitted from every source (``circle.fit_circle``, rounded to
    1/4 px; units whose centres agree still share a launch).
    ``chromatic``: a ``chromatic.ChromaticAberration`` (or one per unit) -- lateral chromatic aberration corrected inside the remap, one
    map per colour channel: channel ``c`` of every result is channel ``c`` of what this call gives for ``transformer *
    PolynomialScaler(coefs_c)``.  uint8 BGR images and lowerable chains only: ValueError (not 3-channel), TypeError (uint16 / float32),
    NotImplementedError (a chain that cannot be lowered), before anything is launched.  ``None``: nothing of it runs.
    ``vignette``: a ``vignette.Vignette`` (or one per unit) -- every source is multiplied by the lens's radial gain in front of the remap
    (and so in front of ``chromatic``), into a temporary: the caller's tensors stay as they are.  The circle is the remap's: this
    ``radius`` and ``center``.  One more launch per source; uint8 and uint16 images (TypeError otherwise, before anything is launched).
    Returns the code path used per launch group ('ray' / 'literal' / 'lut').  Nothing is
    synchronised (``center="auto"`` synchronises once per source)."""
    n = len(srcs)
    if n == 0:
        return []
    if chromatic is not None:
        from . import chromatic as _ca

        _ca.check_images(list(srcs) + list(dsts))
    if vignette is not None:
        from . import vignette as _vg

        _vg.as_per_unit(vignette, n)
        for s_ in srcs:
            _vg.check_dtype(s_.dtype)
    centers = None
    if center is not None:
        centers = per_unit_centers(fit_centers(center, srcs) if isinstance(center, str) else center, n)
    if vignette is not None:
        srcs = _vg.correct_sources(srcs, vignette, centers=centers, radius=radius)
    if chromatic is not None:
        paths, _TLS.plans = _ca.remap_tensors_chromatic(transformer, srcs, dsts, chromatic, radius=radius, interpolation=interpolation,
                                                        boarder_mode=boarder_mode, boarder_value=boarder_value, size_input=size_input,
                                                        rotations=rotations, centers=centers)
        return paths
    if rotations is not None:
        return _remap_with_rotations(transformer, srcs, dsts, rotations, radius=radius, interpolation=interpolation,
                                     boarder_mode=boarder_mode, boarder_value=boarder_value, size_input=size_input, centers=centers)
    # one shared transformer, same geometry and parameters as the previous call: straight to its plan
    # (the key is the chain's exact parameter set, see _param_key, and the shape and pixel type of EVERY unit: a call whose units
    #  differ in either -- the halves of an odd-width frame, images of several types -- needs one plan per kind and never matches
    #  the memo of a call with one kind)
    memo_key = None
    if not isinstance(transformer, (list, tuple)) and len(dsts) == n and isinstance(srcs[0], torch.Tensor) and isinstance(dsts[0], torch.Tensor):
        tk = _transformer_key(transformer)
        if tk is not None and srcs[0].dim() == 3 and dsts[0].dim() == 3:
            try:
                units_key = tuple([(s.shape, s.dtype) for s in srcs] + [(d.shape, d.dtype) for d in dsts])
                memo_key = (tk, float(radius).hex(), units_key, int(interpolation), int(boarder_mode),
                            _border_key(boarder_value, srcs[0].dtype), None if size_input is None else tuple(size_input), srcs[0].device)
                if centers is not None:
                    memo_key += (tuple(centers),)
            except (TypeError, ValueError):
                memo_key = None
            last = _LAST_SHARED[0]  # (one read: another thread may replace the entry at any time)
            if memo_key is not None and last is not None and last[0] == memo_key:
                plan = last[1]
                plan.run(srcs, dsts, None)
                _TLS.plans = [plan]
                return [plan.path_cached]
    dev = srcs[0].device
    for k, (s_, d_) in enumerate(zip(srcs, dsts)):
        if s_.dtype != d_.dtype:
            raise TypeError(f"unit {k}: src {s_.dtype} / dst {d_.dtype}: source and destination must have one pixel type")
    cn = int(srcs[0].shape[2])
    dst_wh = (int(dsts[0].shape[1]), int(dsts[0].shape[0]))
    groups, host_mapped = group_units(transformer, srcs, dsts, radius=radius, size_input=size_input, center=centers)
    paths: list[str] = []
    _TLS.plans = []
    for k, t, size_in_k in host_mapped:
        xm, ym = _host_map(t, radius=radius, size_input=size_in_k, size_output=dst_wh, center=None if centers is None else centers[k])
        xm_d, ym_d = torch.from_numpy(xm).to(dev), torch.from_numpy(ym).to(dev)
        _check_image_tensor(srcs[k], "src")
        _check_image_tensor(dsts[k], "dst")
        if srcs[k].dtype != dsts[k].dtype:
            raise TypeError(f"unit {k}: src {srcs[k].dtype} / dst {dsts[k].dtype}: source and destination must have one pixel type")
        if srcs[k].dtype == torch.uint8:
            bv = border_scalar(boarder_value)
            rc = _native.lib().v1c_remap_lut(
                dev.index, _stream_ptr(dev), srcs[k].data_ptr(), srcs[k].shape[0], srcs[k].shape[1], srcs[k].stride(0), cn,
                dsts[k].data_ptr(), dst_wh[1], dst_wh[0], dsts[k].stride(0), xm_d.data_ptr(), ym_d.data_ptr(),
                xm_d.stride(0) * 4, int(interpolation), int(boarder_mode), bv.ctypes.data,
            )
            _native.check(rc, "v1c_remap_lut")
        else:
            bv = border_scalar_f64(boarder_value)
            es = srcs[k].element_size()
            rc = _native.lib().v1c_remap_lut_ex(
                dev.index, _stream_ptr(dev), srcs[k].data_ptr(), srcs[k].shape[0], srcs[k].shape[1], srcs[k].stride(0) * es, cn,
                DEPTHS[srcs[k].dtype], dsts[k].data_ptr(), dst_wh[1], dst_wh[0], dsts[k].stride(0) * es, xm_d.data_ptr(),
                ym_d.data_ptr(), xm_d.stride(0) * 4, int(interpolation), int(boarder_mode), bv.ctypes.data,
            )
            _native.check(rc, "v1c_remap_lut_ex")
        paths.append("lut")
    for g in groups:
        plan = _plan_for(g.chain, src_hw=g.src_hw, dst_wh=dst_wh, cn=cn, interpolation=interpolation,
                         border_mode=boarder_mode, border_value=boarder_value, device=dev, dtype=g.srcs[0].dtype)
        plan.run(g.srcs, g.dsts, g.rots)
        _TLS.plans.append(plan)
        paths.append(plan.path)
        if memo_key is not None and len(groups) == 1 and not host_mapped and g.rots is None and len(g.srcs) == n:
            plan.path_cached = paths[-1]
            _LAST_SHARED[0] = (memo_key, plan)
    _TLS.plans.extend([_LutLaunch] * len(host_mapped))  # (after the plans' groups: a LUT unit reports 'lut')
    return paths


class LaunchGroup:
    """Units of one call that share a plan: ``chain`` is what the plan is created from (the group's one
    rotation baked in, or blanked when rotations differ per unit and travel in ``rots``)."""

    __slots__ = ("chain", "src_hw", "srcs", "dsts", "rots", "index")

    def __init__(self, chain, src_hw, srcs, dsts, rots, index):
        self.chain, self.src_hw, self.srcs, self.dsts, self.rots, self.index = chain, src_hw, srcs, dsts, rots, index


def group_units(transformer, srcs, dsts, *, radius: float, size_input: tuple[int, int] | None = None, center: Any = None):
    """Host logic of a call, no device involved: lower the chain of every unit (one shared transformer or
    one per unit), split units into groups that share a plan -- same chain up to the matrix of a single
    rotate stage, same source size, same pixel type -- and list the units whose chain cannot be lowered.

    ``center``: one ``(cx, cy)`` or one per unit (``per_unit_centers``); units with different centres have different chains, hence plans.

    Returns ``(groups, host_mapped)``: ``LaunchGroup`` records in first-appearance order and
    ``(unit index, transformer, size_input)`` for units that take the map from their own ``transform()``.
    Used by ``remap_tensors`` and by the multi-GPU dispatcher (sharding.py), whose CPU tests run it as is."""
    n = len(srcs)
    per_unit = list(transformer) if isinstance(transformer, (list, tuple)) else [transformer] * n
    if len(per_unit) != n or len(dsts) != n:
        raise ValueError("need one transformer and one dst per src")
    centers = per_unit_centers(center, n)
    src_hw = (int(srcs[0].shape[0]), int(srcs[0].shape[1]))
    dst_wh = (int(dsts[0].shape[1]), int(dsts[0].shape[0]))
    acc: "OrderedDict[bytes, dict]" = OrderedDict()
    lowered: dict[Any, Any] = {}
    host_mapped = []
    for k, t in enumerate(per_unit):
        # the Denormalize centre is (W_in // 2, H_in // 2) of the image the map is FOR: with one shared
        # transformer that is images[0] (remapper.py:385), with per-eye transformers every eye is its own
        # apply() call and uses its own shape (remapper.py:460-473) -- odd-width SBS files split into W // 2
        # and W - W // 2 columns
        size_in_k = tuple(size_input) if size_input is not None else (
            src_hw if not isinstance(transformer, (list, tuple)) else (int(srcs[k].shape[0]), int(srcs[k].shape[1])))
        c_k = None if centers is None else centers[k]
        lk = (id(t), size_in_k, c_k)
        if lk not in lowered:
            try:
                lowered[lk] = _lower_cached(t, radius=radius, size_input=size_in_k, size_output=dst_wh, center=c_k)
            except NotLowerable as e:
                LOG.warning("transformer chain is not lowerable (%s): map evaluated by its own NumPy transform()", e)
                lowered[lk] = None
        chain = lowered[lk]
        if chain is None:
            host_mapped.append((k, t, size_in_k))
            continue
        shared, rot = _split_single_rotation(chain)
        # different source sizes or pixel types: different plans
        key = bytes(shared) + repr(tuple(srcs[k].shape)).encode() + str(getattr(srcs[k], "dtype", "")).encode()
        g = acc.setdefault(key, {"chain": shared, "full": chain, "src_hw": tuple(int(v) for v in srcs[k].shape[:2]),
                                 "srcs": [], "dsts": [], "rots": [], "index": []})
        g["srcs"].append(srcs[k])
        g["dsts"].append(dsts[k])
        g["rots"].append(rot)
        g["index"].append(k)
    groups = []
    for g in acc.values():
        # one rotation for the whole group (or none): bake it into the plan, which then computes its
        # tile boxes once and shares coordinates between units; rotations that differ per unit
        # travel with the units and share the rotation-blanked plan
        r0 = g["rots"][0]
        uniform = r0 is None or all(np.array_equal(r, r0) for r in g["rots"])
        groups.append(LaunchGroup(g["full"] if uniform else g["chain"], g["src_hw"], g["srcs"], g["dsts"],
                                  None if uniform else g["rots"], g["index"]))
    return groups, host_mapped


def _remap_with_rotations(transformer, srcs, dsts, rotations, *, radius, interpolation, boarder_mode, boarder_value, size_input, centers=None):
    from .quat import as_rotation_matrix

    if isinstance(transformer, (list, tuple)) or len(rotations) != len(srcs) or len(dsts) != len(srcs):
        raise ValueError("rotations= needs ONE transformer chain and one rotation / dst per src")
    dev = srcs[0].device
    src_hw = (int(srcs[0].shape[0]), int(srcs[0].shape[1]))
    dst_wh = (int(dsts[0].shape[1]), int(dsts[0].shape[0]))
    if centers is not None and any(c != centers[0] for c in centers):
        raise ValueError("rotations= shares one plan: it takes ONE center for all units")
    chain = lower_for_get_map(transformer, radius=radius, size_input=size_input or src_hw, size_output=dst_wh,
                              center=None if centers is None else centers[0])
    shared, rot = _split_single_rotation(chain)
    if rot is None:
        raise ValueError("rotations= needs a chain with exactly one Euclidean3DRotator")
    plan = _plan_for(shared, src_hw=src_hw, dst_wh=dst_wh, cn=int(srcs[0].shape[2]), interpolation=interpolation,
                     border_mode=boarder_mode, border_value=boarder_value, device=dev, dtype=srcs[0].dtype)
    plan.run(srcs, dsts, [as_rotation_matrix(r) for r in rotations])
    _TLS.plans = [plan]
    return [plan.path]


# --------------------------------------------------------------------------------------------
# reference API
# --------------------------------------------------------------------------------------------
def get_map(
    transformer: TransformerBase,
    *,
    radius: float,
    size_input: tuple[int, int],
    size_output: tuple[int, int] = (2048, 2048),
    device: Any = None,
    center: Any = None,
    chromatic: Any = None,
    channel: str | None = None,
) -> tuple[NDArray[np.float32], NDArray[np.float32]]:
    """Generate the remap map (reference remapper.py:23-59): float32 ``xmap, ymap`` of shape
    ``(size_output[1], size_output[0])``.  Evaluated on the GPU by the same code the fused kernel
    uses; non-lowerable chains are evaluated through their own ``transform`` like the reference.
    ``center`` = (cx, cy): the image circle's centre instead of ``(W_in // 2, H_in // 2)`` (``"auto"`` needs an image: ValueError).
    ``chromatic`` with ``channel`` = "b" / "g" / "r": that channel's map under a ``chromatic.ChromaticAberration``."""
    if chromatic is not None or channel is not None:
        from . import chromatic as _ca

        if chromatic is None or channel is None:
            raise ValueError('get_map: chromatic= and channel= ("b", "g" or "r") go together')
        return _ca.get_map_channel(transformer, chromatic, channel, radius=radius, size_input=size_input, size_output=size_output,
                                   device=device, center=center)
    try:
        chain = lower_for_get_map(transformer, radius=radius, size_input=size_input, size_output=size_output, center=center)
    except NotLowerable:
        return _host_map(transformer, radius=radius, size_input=size_input, size_output=size_output, center=center)
    plan = _plan_for(chain, src_hw=(max(1, size_input[0]), max(1, size_input[1])), dst_wh=size_output, cn=3,
                     interpolation=_abi.INTER_LINEAR, border_mode=BORDER_CONSTANT, border_value=0, device=device)
    xm, ym = plan.get_map()
    return xm.cpu().numpy(), ym.cpu().numpy()


def _capturing() -> bool:
    return bool(torch.cuda.is_available() and torch.cuda.is_current_stream_capturing())


def _is_center_pair(c: Any) -> bool:
    return (isinstance(c, (tuple, list, np.ndarray)) and len(c) == 2
            and all(isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) for v in c))


def per_unit_centers(center: Any, n: int) -> list | None:
    """``center=`` of a call with ``n`` units as one entry per unit: ``None`` (every unit keeps ``(W_in // 2, H_in // 2)``), else a list
    of ``(cx, cy)`` float pairs and ``None`` entries.  Takes ``None``, one pair, or a sequence of ``n`` pairs / ``None``."""
    if center is None:
        return None
    if isinstance(center, str):
        raise ValueError(f"center={center!r}: resolve it from the images first (fit_centers)")
    if _is_center_pair(center):
        return [(float(center[0]), float(center[1]))] * n
    cs = list(center)
    if len(cs) != n or not all(c is None or _is_center_pair(c) for c in cs):
        raise ValueError(f"center must be (cx, cy) or one (cx, cy) / None per image ({n})")
    out = [None if c is None else (float(c[0]), float(c[1])) for c in cs]
    return None if all(c is None for c in out) else out


def fit_circles(images: Sequence[Any], device: Any = None) -> list:
    """``circle.fit_circle`` of every image (one synchronisation each); ValueError where an image has no circle"""
    from . import circle

    return [circle.fit_circle(im, device=device) for im in images]


def fit_centers(center: str, images: Sequence[Any], device: Any = None, fits: Sequence[Any] | None = None) -> list[tuple[float, float]]:
    """``center="auto"``: the fitted centre of every image, each its own, rounded to 1/4 px (the fit is not better than that on real
    rims, and the frames of one rig then share their plans).  NotImplementedError while the stream is being captured: the plan's tile
    boxes depend on the centre, which has to visit the host."""
    from . import circle

    if center != "auto":
        raise ValueError(f'center must be None, (cx, cy), one per image or "auto", not {center!r}')
    if _capturing():
        raise NotImplementedError('center="auto" cannot be captured into a graph (the fitted centre visits the host); pass explicit centres')
    fits = fit_circles(images, device) if fits is None else fits
    return [circle.round_center(f.cx, f.cy) for f in fits]


def get_radius_smart(radius: float | Literal["auto", "max", "fit"], images: Sequence[Any], *, fits: Sequence[Any] | None = None,
                     device: Any = None) -> float:
    """Reference remapper.py:62-90.  ``images`` may be numpy arrays or device tensors.
    ``"fit"`` (not in the reference): the radius of the fitted image circle (``circle.fit_circle``; ``fits``: the fits where the caller
    has them already), the maximum over the images, rounded to 1/2 px -- ``get_radius``'s own grid.  It is POSITIVE: it deliberately
    does not reproduce the sign quirk of ``"auto"``, whose estimate is negative on an image circle on black (the 180-degree flip of the
    map)."""
    if isinstance(radius, str) and radius == "fit":
        from . import circle

        radius_ = max(circle.round_radius(f.radius) for f in (fit_circles(images, device) if fits is None else fits))
    elif isinstance(radius, str) and radius == "auto":
        radius_ = max(_get_radius_any(im) for im in images)
    elif isinstance(radius, str) and radius == "max":
        radius_ = min(images[0].shape[0] / 2, images[0].shape[1] / 2)
    else:
        radius_ = radius
    if LOG.isEnabledFor(logging.INFO):
        LOG.info(f"Radius: {radius_}, strategy: {radius}, image shape: {tuple(images[0].shape)}")
    return radius_


def _get_radius_any(im: Any, threshold: int = 10) -> float:
    if isinstance(im, torch.Tensor) and im.is_cuda and im.dtype != torch.uint8:
        # 16-bit / float32 on the device: the scan kernel is 8-bit; the centre row (landscape) or column (transformer.py:126-129) is all
        # the estimate reads -- it alone comes to the host, as a (1, W, C) / (H, 1, C) image with the same centre line
        _check_image_tensor(im, "image")
        h, w = int(im.shape[0]), int(im.shape[1])
        line = im[h // 2][None] if w > h else im[:, w // 2][:, None]
        return float(get_radius(line.cpu().numpy(), threshold=threshold))
    if isinstance(im, torch.Tensor) and im.is_cuda:
        _check_image_tensor(im, "image")
        r = C.c_double()
        rc = _native.lib().v1c_get_radius(im.device.index, _stream_ptr(im.device), im.data_ptr(), im.shape[0], im.shape[1],
                                          im.stride(0), im.shape[2], threshold, C.byref(r))
        if rc == _abi.E_INVALID and b"no black border" in _native.lib().v1c_last_error():
            raise IndexError("index 0 is out of bounds for axis 0 with size 0")  # what the reference raises
        _native.check(rc, "v1c_get_radius")
        return r.value
    return float(get_radius(np.asarray(im), threshold=threshold))


def _to_device(img: Any, dev: torch.device) -> torch.Tensor:
    if isinstance(img, torch.Tensor):
        return img if img.device == dev else img.to(dev)
    a = np.asarray(img)
    if a.dtype not in NP_DTYPES:
        raise TypeError(f"images must be uint8, uint16 or float32, not {a.dtype}")  # cv2.remap's CV_8U / CV_16U / CV_32F
    if a.ndim == 2:
        a = a[..., None]
    # column-sliced views (remapper.py:455-456) are made contiguous on the host before upload; read-only arrays
    # (memory-mapped .npy frames, Pillow buffers) are copied: torch refuses to alias them silently
    a = np.ascontiguousarray(a) if a.flags.writeable else np.array(a, order="C")
    return torch.from_numpy(a).to(dev, non_blocking=False)


def _decode_on_device(items: Sequence[Any], device: Any, mode: Any = True, progressive: bool = False) -> list:
    """``device_decode=True``: jpeg_decode_device.read_inputs -- ``.jpg`` / ``.jpeg`` paths decoded on the device, everything else and
    files the device decoder does not take left for ``_io.imread``; ``device_decode="batch"``: the same through one batched decode;
    ``progressive`` (``device_decode_progressive``): progressive files stay on the device too"""
    from . import jpeg_decode_device

    if isinstance(mode, str) and mode != "batch":
        raise ValueError('device_decode must be True, False or "batch"')
    kw: dict = {"progressive": True} if progressive else {}
    if mode == "batch":
        return jpeg_decode_device.read_inputs(items, device=device, batch=True, **kw)
    return jpeg_decode_device.read_inputs(items, device=device, **kw)


def _device_jpeg_mode(mode: Any) -> Any:
    """``device_jpeg``: False, True (a call of the device encoder per result) or ``"batch"`` (one call for all of them)"""
    if isinstance(mode, str) and mode != "batch":
        raise ValueError('device_jpeg must be True, False or "batch"')
    return mode


def apply(
    transformer: TransformerBase,
    *,
    in_paths: Sequence[Path | str | NDArray] | Path | str | NDArray,
    out_paths: Sequence[Path | str] | None | Path | str = None,
    size_output: tuple[int, int] = (2048, 2048),
    interpolation: int = INTER_LANCZOS4,
    boarder_mode: int = BORDER_CONSTANT,
    boarder_value: int | tuple[int, int, int] = 0,
    radius: float | Literal["auto", "max"] = "auto",
    device: Any = None,
    device_png: bool = False,
    device_jpeg: bool | Literal["batch"] = False,
    device_decode: bool | Literal["batch"] = False,
    device_jpeg_optimize: bool = False,
    device_decode_progressive: bool = False,
    center: Any = None,
    chromatic: Any = None,
    vignette: Any = None,
) -> Sequence[NDArray[np.uint8]]:
    """Apply transformer to images (reference remapper.py:324-403).

    Returns one ``(size_output[1], size_output[0], C)`` array per input, of the input's pixel type
    (uint8, uint16 or float32; CUDA tensors in -> CUDA tensors out).  One map is shared by all
    images and, like the reference, takes its geometry from ``images[0]``; images of different
    pixel types are remapped by one plan per type.

    ``device_decode=True``: ``.jpg`` / ``.jpeg`` inputs are decoded on the device (jpeg_decode_device.py) and take the device-resident
    route -- with anything that came from the host reader uploaded to join them --, so the results are CUDA tensors; files outside the
    device decoder's scope are read by the host as before.  ``device_decode="batch"``: the same, with all the files decoded in one
    batch that shares its launches and synchronisation rounds (jpeg_decode_device.decode_jpeg_tensors).

    ``device_jpeg=True``: every ``.jpg`` / ``.jpeg`` result that is a uint8 tensor on the device is encoded there, one call of the
    encoder per result (jpeg_device.imwrite_jpeg_tensor).  ``device_jpeg="batch"``: all of them in ONE call that shares its launches
    and its two synchronisations (jpeg_device.imwrite_jpeg_tensors); the files are the same bytes.  The other results take the paths
    they take without it (``device_png``, the host writer).  ``device_jpeg_optimize=True``: those files get Huffman tables built for
    each image on the device (``optimize=True`` of jpeg_device.py: smaller files, the same pixels) with either ``device_jpeg`` mode;
    it does nothing without one.  ``device_decode_progressive=True``: with either ``device_decode`` mode, progressive JPEG inputs are
    decoded on the device too (``progressive=True`` of jpeg_decode_device.py; under ``"batch"`` each by a call of its own behind the
    batch) instead of going to the host reader; it does nothing without ``device_decode``.

    ``center``: the image circle's centre in source pixels instead of ``(W_in // 2, H_in // 2)`` -- ``(cx, cy)`` for all images, one
    per image, or ``"auto"``: every image's own, fitted on the device (circle.py) and rounded to 1/4 px.  ``radius="fit"``: the fitted
    radius (``get_radius_smart``); the radius stays shared, the maximum over the images, whatever the centres.

    ``chromatic``: a ``chromatic.ChromaticAberration`` -- lateral chromatic aberration corrected inside the remap, one map per colour
    channel (``remap_tensors``); uint8 BGR images and lowerable chains only, refused before anything is launched.

    ``vignette``: one ``vignette.Vignette`` -- every image is multiplied by the lens's radial gain in front of the remap, with the
    remap's circle (``radius``, ``center``); arrays and tensors of the caller's stay as they are, images this call read or decoded
    itself are corrected where they lie.  uint8 and uint16 images, TypeError otherwise, before anything is launched."""
    device_jpeg = _device_jpeg_mode(device_jpeg)
    jpeg_kw = {"optimize": True} if device_jpeg_optimize else {}
    in_paths_ = [in_paths] if isinstance(in_paths, (str, Path, np.ndarray, torch.Tensor)) else in_paths
    out_paths_ = [out_paths] if isinstance(out_paths, (str, Path)) else out_paths
    del in_paths, out_paths

    caller_items = list(in_paths_)
    if device_decode:
        in_paths_ = _decode_on_device(list(in_paths_), device, device_decode, device_decode_progressive)
    images = _io.imread_many(list(in_paths_))
    if device_decode:
        decoded = next((im for im in images if isinstance(im, torch.Tensor) and im.is_cuda), None)
        if decoded is not None:
            images = [_to_device(im, decoded.device) for im in images]
    ca_kw: dict = {}
    if chromatic is not None:
        from . import chromatic as _ca

        if not isinstance(chromatic, _ca.ChromaticAberration):  # (one map serves every image: one correction)
            raise TypeError(f"apply: chromatic must be one ChromaticAberration, not {chromatic!r}")
        _ca.check_images(images)
        ca_kw = {"chromatic": chromatic}
    if vignette is not None:
        from . import vignette as _vg

        if not isinstance(vignette, _vg.Vignette):  # (one map serves every image: one correction)
            raise TypeError(f"apply: vignette must be one Vignette, not {vignette!r}")
        for im in images:
            _vg.check_dtype(im.dtype)
    fits = None
    if (isinstance(radius, str) and radius == "fit") or isinstance(center, str):
        if isinstance(center, str) and _capturing():
            fit_centers(center, images)  # (raises)
        fits = fit_circles(images, device)
    radius_ = get_radius_smart(radius, images) if fits is None else get_radius_smart(radius, images, fits=fits)
    centers = per_unit_centers(fit_centers(center, images, fits=fits) if isinstance(center, str) else center, len(images))
    if centers is not None and all(c == centers[0] for c in centers):
        center_ = centers[0]  # one centre for all: every route below takes it as it takes the radius
    else:
        center_ = centers
    on_device = all(isinstance(im, torch.Tensor) and im.is_cuda for im in images)
    dev = images[0].device if on_device else _device(device)

    # host-resident batch: copies in, remap and copies out of different groups overlap (_hostpipe.py)
    host_imgs = None if on_device else [np.asarray(im) if not isinstance(im, torch.Tensor) else None for im in images]
    if (host_imgs is not None and _hostpipe.enabled(len(images), len(images) * size_output[0] * size_output[1] * 4) and all(a is not None and a.dtype == np.uint8 and a.ndim in (2, 3)
                                                                        and a.shape == host_imgs[0].shape for a in host_imgs)
            and boarder_mode != _abi.BORDER_TRANSPARENT and (center_ is None or _is_center_pair(center_))):
        imgs3 = [a[..., None] if a.ndim == 2 else a for a in host_imgs]
        size_in = (int(imgs3[0].shape[0]), int(imgs3[0].shape[1]))

        def _group(srcs_g, dsts_g):
            remap_tensors(transformer, srcs_g, dsts_g, radius=radius_, interpolation=interpolation, boarder_mode=boarder_mode,
                          boarder_value=boarder_value, size_input=size_in, center=center_, **ca_kw,
                          **({} if vignette is None else {"vignette": vignette}))

        results = _hostpipe.run(imgs3, dev, (size_output[1], size_output[0], int(imgs3[0].shape[2])), _group)
        results = [r[..., 0] if a.ndim == 2 else r for r, a in zip(results, host_imgs)]
        if out_paths_ is not None:
            _io.imwrite_many(list(out_paths_)[: len(results)], results)
        return results

    srcs = [_to_device(im, dev) for im in images]
    if vignette is not None:  # (in place where the tensor is this call's own: an upload or a decode; never in the caller's)
        srcs = _vg.correct_sources(srcs, vignette, centers=centers, radius=radius_,
                                   inplace=[not isinstance(q, torch.Tensor) for q in caller_items])
    cn = srcs[0].shape[2]
    dsts = [torch.empty((size_output[1], size_output[0], cn), dtype=s.dtype, device=dev) for s in srcs]
    if boarder_mode == _abi.BORDER_TRANSPARENT:
        for d in dsts:  # cv2 leaves skipped pixels uninitialised; make them deterministic
            d.zero_()
    remap_tensors(transformer, srcs, dsts, radius=radius_, interpolation=interpolation, boarder_mode=boarder_mode,
                  boarder_value=boarder_value, size_input=(int(srcs[0].shape[0]), int(srcs[0].shape[1])), center=center_, **ca_kw)
    if on_device:
        results: list[Any] = dsts
    else:
        results = [d.cpu().numpy() for d in dsts]
        results = [r[..., 0] if np.asarray(im).ndim == 2 else r for r, im in zip(results, images)]
    if out_paths_ is not None:
        paths = list(out_paths_)[: len(results)]
        if device_png or device_jpeg:
            writers = []  # .png / .jpg results still on the device are encoded there (png_device.py, jpeg_device.py)
            if device_png:
                from . import png_device

                writers.append((png_device.eligible, png_device.imwrite_tensor))
            if device_jpeg:
                from . import jpeg_device

                writers.append((jpeg_device.eligible, jpeg_device.imwrite_jpeg_tensor))
            on_dev = [next((write for ok, write in writers if ok(q, d)), None) for q, d in zip(paths, dsts)]
            if device_jpeg == "batch":  # the eligible results in one call, in order; the writer above only marks them
                together = [i for i, write in enumerate(on_dev) if write is jpeg_device.imwrite_jpeg_tensor]
                if together:
                    jpeg_device.imwrite_jpeg_tensors([paths[i] for i in together], [dsts[i] for i in together], **jpeg_kw)
            for q, d, write in zip(paths, dsts, on_dev):
                if write and not (device_jpeg == "batch" and write is jpeg_device.imwrite_jpeg_tensor):
                    write(q, d, **(jpeg_kw if device_jpeg and write is jpeg_device.imwrite_jpeg_tensor else {}))
            keep = [i for i, ok in enumerate(on_dev) if not ok]
            paths, results_ = [paths[i] for i in keep], [results[i] for i in keep]
        else:
            results_ = results
        _io.imwrite_many(paths, [image.cpu().numpy() if isinstance(image, torch.Tensor) else image for image in results_])
    return results


def auto_radius_tensor(images: Sequence[torch.Tensor], threshold: int = 10) -> torch.Tensor:
    """``get_radius`` (transformer.py:108-140) of every image, left on the device: a float64 ``(n, 2)`` tensor of (radius, status) pairs
    (``v1c_get_radius_async``; status 1.0 / radius NaN where the reference raises IndexError).  Current stream, nothing synchronised."""
    dev = images[0].device
    rad = torch.empty((len(images), 2), dtype=torch.float64, device=dev)
    for k, im in enumerate(images):
        _check_image_tensor(im, "image")
        if im.dtype != torch.uint8:  # (the scan kernel reads bytes; 16-bit / float32: _get_radius_any, on the host)
            raise TypeError(f"auto_radius_tensor: uint8 images only, not {im.dtype}")
        rc = _native.lib().v1c_get_radius_async(dev.index, _stream_ptr(dev), im.data_ptr(), im.shape[0], im.shape[1], im.stride(0), im.shape[2],
                                                threshold, rad.data_ptr() + 16 * k)
        _native.check(rc, "v1c_get_radius_async")
    return rad


def remap_tensors_auto(transformer: TransformerBase, srcs: Sequence[torch.Tensor], dsts: Sequence[torch.Tensor], *,
                       rad: torch.Tensor | None = None, interpolation: int = INTER_LANCZOS4, boarder_mode: int = BORDER_CONSTANT,
                       boarder_value: Any = 0, size_input: tuple[int, int] | None = None, center: Any = None) -> None:
    """``remap_tensors`` with ``radius="auto"`` -- the reference's default, remapper.py:333 -- and the radius never leaving the device:
    estimated from ``srcs`` (or given as ``rad``, ``auto_radius_tensor``), the maximum taken and the Denormalize scale set by ONE small
    launch in front of the remap launch (``v1c_plan_run_auto_images`` / ``v1c_plan_run_auto``).  No stream synchronisation, no
    plan per image (ONE plan serves every radius: it is keyed on the nominal radius "max"), graph-capturable once the plan exists.
    Where the reference raises IndexError (an image without a black border) the map is sent to the Denormalize centre -40000 px
    (scale 0): every pixel samples there under the border mode -- BORDER_CONSTANT the border colour, BORDER_TRANSPARENT leaves ``dsts``
    untouched, REPLICATE / REFLECT / WRAP / REFLECT_101 what those modes read at (-40000, -40000).
    Sources of different shapes (the halves of an odd-width side-by-side frame) share the map of ``srcs[0]``'s geometry, like
    ``remap_tensors``: one radius over all of them (``auto_radius_tensor``), one launch per source shape (``auto_groups``).
    Raises NotImplementedError for chains the device-resident form does not serve (see include/vr180_remap.h), chains that cannot be
    lowered among them; a decline after the first of several shape groups has run leaves that group's outputs written (with the very
    bytes the caller's fallback writes again).
    ``center`` = (cx, cy): ONE explicit image-circle centre for every source instead of ``(W_in // 2, H_in // 2)`` (a fitted one would
    have to visit the host: ``center="auto"`` is refused)."""
    if center is not None and not _is_center_pair(center):
        raise NotImplementedError("remap_tensors_auto takes ONE explicit center (cx, cy): the plan's boxes depend on it")
    if isinstance(transformer, (list, tuple)):
        raise ValueError("remap_tensors_auto takes ONE transformer (per-eye transformers: one call per eye, as apply_lr does)")
    if any(s.dtype != torch.uint8 for s in srcs):
        # (the device-resident radius is 8-bit only: 16-bit / float32 images take the exact form, the estimate on the host)
        raise NotImplementedError("remap_tensors_auto: 8-bit images only (16-bit / float32: the radius goes to the host)")
    dev = srcs[0].device
    src_hw = (int(srcs[0].shape[0]), int(srcs[0].shape[1]))
    dst_wh = (int(dsts[0].shape[1]), int(dsts[0].shape[0]))
    size_in = tuple(size_input) if size_input is not None else src_hw
    nominal = min(size_in[0] / 2, size_in[1] / 2)  # (any radius: the launch ignores the plan's own)
    try:
        chain = _lower_cached(transformer, radius=nominal, size_input=size_in, size_output=dst_wh,
                              center=None if center is None else (float(center[0]), float(center[1])))
    except NotLowerable as e:  # (the callers' fallback, remap_tensors, serves it from the chain's own transform(): the LUT path)
        raise NotImplementedError(f"remap_tensors_auto: the chain cannot be lowered ({e})") from e
    groups = auto_groups(srcs)
    if len(groups) > 1 and rad is None:
        rad = auto_radius_tensor(srcs)  # (ONE radius over every source: the scan launch of run_auto only sees its own group)
    plans = []
    for hw, idx in groups:
        plan = _plan_for(chain, src_hw=hw, dst_wh=dst_wh, cn=int(srcs[0].shape[2]), interpolation=interpolation,
                         border_mode=boarder_mode, border_value=boarder_value, device=dev)
        # (rad None: the call estimates from `srcs` itself -- one small launch in front of the remap)
        plan.run_auto([srcs[k] for k in idx], [dsts[k] for k in idx], rad)
        plans.append(plan)
    _TLS.plans = plans
    _TLS.auto_form = "device"


def auto_groups(srcs: Sequence[Any]) -> list[tuple[tuple[int, int], list[int]]]:
    """How ``remap_tensors_auto`` splits its units: ``(source (H, W), unit indices)`` per distinct source shape, in first-appearance
    order (a ``v1c_plan`` is made for one source size).  Host logic only: shapes are read, no device is touched."""
    acc: "OrderedDict[tuple[int, int], list[int]]" = OrderedDict()
    for k, s in enumerate(srcs):
        acc.setdefault((int(s.shape[0]), int(s.shape[1])), []).append(k)
    return list(acc.items())


def _remap_host_radius(transformer: TransformerBase, srcs, dsts, r: float, *, interpolation, boarder_mode, boarder_value, size_input) -> bool:
    """``radius="auto"`` with the estimate taken to the host (the exact form: IndexError like the reference), for an image circle that
    moved: the launch that reads the radius from device memory (``v1c_plan_run_auto``: one plan whatever the radius, the kernels
    without plan-time boxes) instead of a plan per radius -- 0.2 ms instead of 0.6 - 1.2 ms of plan creation per new radius.  A
    circle that repeats (the same estimate twice in a row) gets its own plan and the planned kernels.  Same bytes either way.
    False: not served (chains the device-resident launch does not take, a repeated radius) -- the caller runs the planned path."""
    k = _transformer_key(transformer)
    if k is None or any(s.dtype != torch.uint8 for s in srcs):
        return False
    dev = srcs[0].device
    key = (k, tuple(size_input), tuple(int(v) for v in dsts[0].shape[:2]), int(srcs[0].shape[2]), int(interpolation), int(boarder_mode),
           border_scalar(boarder_value).tobytes(), dev.index)
    with _PLANS_LOCK:
        last = _AUTO_LAST.get(key)
        _AUTO_LAST[key] = r
        while len(_AUTO_LAST) > 64:
            _AUTO_LAST.pop(next(iter(_AUTO_LAST)))
    if last == r:
        return False
    try:
        rad = torch.tensor([[r, 0.0]], dtype=torch.float64, device=dev)
        remap_tensors_auto(transformer, srcs, dsts, rad=rad, interpolation=interpolation, boarder_mode=boarder_mode, boarder_value=boarder_value,
                           size_input=size_input)
        _TLS.auto_form = "exact"  # (the estimate did visit the host)
        return True
    except NotImplementedError:
        return False


def apply_lr_tensors(
    transformer: TransformerBase | tuple[TransformerBase, TransformerBase],
    left: torch.Tensor,
    right: torch.Tensor,
    *,
    out: torch.Tensor | None = None,
    size_output: tuple[int, int] = (2048, 2048),
    interpolation: int = INTER_LANCZOS4,
    boarder_mode: int = BORDER_CONSTANT,
    boarder_value: Any = 0,
    radius: float | Literal["auto", "max"] = "auto",
    auto_radius_on_device: bool | None = None,
    center: Any = None,
    match_colors: Literal["gain", "histogram"] | None = None,
    match_reference: Literal["left", "right"] = "left",
    chromatic: Any = None,
    vignette: Any = None,
) -> torch.Tensor:
    """Device-resident ``apply_lr`` (merge=False): both eyes are remapped by ONE launch straight
    into the halves of the ``(H, 2W, C)`` side-by-side tensor (remapper.py:460-484, 517-518).

    ``radius="auto"`` (the reference's default) has two forms.  The exact one brings each estimate to the host (one stream
    synchronisation; raises IndexError like the reference when an image has no black border; a circle that moved is served by the
    launch that reads the radius from device memory -- no plan per radius --, a circle that repeats by a plan of its own).
    ``auto_radius_on_device=True`` keeps it on the device (``remap_tensors_auto``): no synchronisation, one plan for every radius,
    graph-capturable; default (None): taken when the current stream is being captured into a graph, where a synchronisation is illegal.

    uint16 / float32 eyes give an output of their type.  Their radius="auto" always takes the exact form (the device-resident one is
    8-bit only): under graph capture with ``auto_radius_on_device=None`` the NotImplementedError of ``remap_tensors_auto`` propagates,
    as it does for chains that form does not serve -- pass a numeric radius there.

    ``center``: the image circles' centres in source pixels instead of ``(W_in // 2, H_in // 2)`` -- one ``(cx, cy)`` for both eyes,
    ``((lx, ly), (rx, ry))`` per eye (each in its own eye's coordinates), or ``"auto"``: each eye's own, fitted on the device and rounded
    to 1/4 px (circle.py).  Eyes whose centres differ are remapped by a launch each.  ``"auto"`` needs the fitted centres on the host
    (the plan's tile boxes depend on them): NotImplementedError under stream capture and with ``auto_radius_on_device=True``; explicit
    centres work in both.  ``radius="fit"``: the fitted radius (``get_radius_smart``), positive; ``radius="auto"`` keeps its value,
    sign included, whatever ``center``.

    ``match_colors``: ``"gain"`` or ``"histogram"`` -- after the remap, the half that is not ``match_reference`` is rewritten in place so
    that its colours match the other half's (colormatch.py; three more launches on the current stream, nothing synchronised, so it goes
    into a graph capture with the remap).  uint8 eyes only: ValueError before anything is remapped.  None: nothing of it runs.

    ``chromatic``: a ``chromatic.ChromaticAberration`` for both eyes -- one launch of two units -- or ``(left, right)``, one per eye: two
    plans.  Lateral chromatic aberration corrected inside the remap, one map per colour channel (``remap_tensors``).  uint8 BGR eyes and
    lowerable chains only; ``radius="auto"`` takes its exact form (``auto_radius_on_device=True``: NotImplementedError).  All refused
    before anything is launched.  None: nothing of it runs.

    ``vignette``: a ``vignette.Vignette`` for both eyes or ``(left, right)``, one per eye -- each eye is multiplied by its lens's radial
    gain in front of the remap (and so in front of ``chromatic`` and ``match_colors``), into a temporary: the caller's tensors stay as
    they are.  The circle is the remap's: ``center`` (``"auto"`` included) and ``radius`` -- a number, ``"max"``, ``"fit"`` or the
    exact form of ``"auto"``, resolved ONCE, on the eyes as they came, and used by both (``auto_radius_on_device=True``: the radius
    never reaches the host, NotImplementedError).  One more launch per eye; uint8 and uint16 eyes, TypeError otherwise; all refused
    before anything is launched.  None: nothing of it runs."""
    if vignette is not None:
        left, right, radius, center = _vignette_pair(transformer, left, right, vignette, radius=radius, center=center,
                                                     auto_radius_on_device=auto_radius_on_device)
    ca_kw: dict = {}
    if chromatic is not None:
        from . import chromatic as _ca

        _ca.as_per_unit(chromatic, 2)
        _ca.check_images([left, right])
        if auto_radius_on_device:
            raise NotImplementedError("chromatic: the device-resident radius=\"auto\" form is not served; pass auto_radius_on_device=None "
                                      "(the exact form) or a numeric radius")
        ca_kw = {"chromatic": chromatic}
    if match_colors is not None:
        _check_match_colors(match_colors, match_reference, left, right)
        out = apply_lr_tensors(transformer, left, right, out=out, size_output=size_output, interpolation=interpolation,
                               boarder_mode=boarder_mode, boarder_value=boarder_value, radius=radius,
                               auto_radius_on_device=auto_radius_on_device, center=center, **ca_kw)
        from . import colormatch

        colormatch.match_eyes_tensors(out[:, : size_output[0]], out[:, size_output[0]:], mode=match_colors, reference=match_reference)
        return out
    w, h = size_output
    cn = left.shape[2]
    fits = None
    if isinstance(center, str):
        if auto_radius_on_device:
            raise NotImplementedError('center="auto" takes the fitted centres to the host: it does not go with auto_radius_on_device=True')
        fits = None if _capturing() else fit_circles([left, right])
        center = fit_centers(center, [left, right], fits=fits)
    elif isinstance(radius, str) and radius == "fit":
        fits = fit_circles([left, right])
    centers = per_unit_centers(center, 2)
    same_center = centers is None or centers[0] == centers[1]
    if out is None:
        out = torch.empty((h, 2 * w, cn), dtype=left.dtype, device=left.device)
        if boarder_mode == _abi.BORDER_TRANSPARENT:
            out.zero_()
    halves = [out[:, :w], out[:, w:]]
    if isinstance(radius, str) and radius == "auto":
        on_dev = auto_radius_on_device
        if on_dev is None:
            on_dev = bool(torch.cuda.is_current_stream_capturing())
        if on_dev and not ca_kw:
            try:
                if isinstance(transformer, tuple):  # per-eye transformer AND per-eye radius (remapper.py:460-473)
                    for k, (t, im, d) in enumerate(zip(transformer, (left, right), halves)):
                        remap_tensors_auto(t, [im], [d], interpolation=interpolation, boarder_mode=boarder_mode, boarder_value=boarder_value,
                                           center=None if centers is None else centers[k])
                elif same_center:
                    remap_tensors_auto(transformer, [left, right], halves, interpolation=interpolation, boarder_mode=boarder_mode,
                                       boarder_value=boarder_value, size_input=(int(left.shape[0]), int(left.shape[1])),
                                       center=None if centers is None else centers[0])
                else:  # a centre per eye: a launch per eye, ONE radius over both (the maximum, as get_radius_smart has it)
                    if left.dtype != torch.uint8 or right.dtype != torch.uint8:
                        raise NotImplementedError("remap_tensors_auto: 8-bit images only (16-bit / float32: the radius goes to the host)")
                    rad = auto_radius_tensor([left, right])
                    for k, (im, d) in enumerate(zip((left, right), halves)):
                        remap_tensors_auto(transformer, [im], [d], rad=rad, interpolation=interpolation, boarder_mode=boarder_mode,
                                           boarder_value=boarder_value, size_input=(int(left.shape[0]), int(left.shape[1])), center=centers[k])
                _TLS.auto_form = "device"
                return out
            except NotImplementedError:
                if auto_radius_on_device is None and torch.cuda.is_current_stream_capturing():
                    raise
                # (this chain is not served by the device-resident form: the exact one below)
        _TLS.auto_form = "exact"
    if isinstance(transformer, tuple):
        # per-eye transformer AND per-eye radius estimate (remapper.py:460-473)
        r = list(radius) if isinstance(radius, tuple) else [
            get_radius_smart(radius, [im]) if fits is None else get_radius_smart(radius, [im], fits=[f])
            for im, f in zip((left, right), fits or (None, None))]  # (a tuple: what _vignette_pair resolved per eye)
        if r[0] == r[1]:
            remap_tensors(list(transformer), [left, right], halves, radius=r[0], interpolation=interpolation,
                          boarder_mode=boarder_mode, boarder_value=boarder_value, center=centers, **ca_kw)
        else:
            for k, (t, im, d, rr) in enumerate(zip(transformer, (left, right), halves, r)):
                ca_k = {"chromatic": _ca.as_per_unit(chromatic, 2)[k]} if ca_kw else {}
                remap_tensors(t, [im], [d], radius=rr, interpolation=interpolation, boarder_mode=boarder_mode,
                              boarder_value=boarder_value, center=None if centers is None else centers[k], **ca_k)
    else:
        r_ = get_radius_smart(radius, [left, right]) if fits is None else get_radius_smart(radius, [left, right], fits=fits)
        size_in = (int(left.shape[0]), int(left.shape[1]))
        if centers is not None or ca_kw:  # (the launch that reads a moved radius from device memory is keyed without a centre: the planned path)
            remap_tensors(transformer, [left, right], halves, radius=r_, interpolation=interpolation,
                          boarder_mode=boarder_mode, boarder_value=boarder_value, size_input=size_in, center=centers, **ca_kw)
        elif not (isinstance(radius, str) and radius == "auto" and
                _remap_host_radius(transformer, [left, right], halves, float(r_), interpolation=interpolation, boarder_mode=boarder_mode,
                                   boarder_value=boarder_value, size_input=size_in)):
            remap_tensors(transformer, [left, right], halves, radius=r_, interpolation=interpolation,
                          boarder_mode=boarder_mode, boarder_value=boarder_value, size_input=size_in)
    return out


def _vignette_pair(transformer, left, right, vignette, *, radius, center, auto_radius_on_device=None, inplace=(False, False)):
    """``vignette=`` of the pair entries: the circle resolved as the remap resolves it -- once, on the eyes as they came --, both eyes
    corrected (vignette.py; ``inplace[k]``: where eye k lies), and what the remap is then called with: ``(left, right, radius,
    center)``.  ``radius`` comes back as a number, or as ``(r_left, r_right)`` where a transformer per eye takes a radius per eye."""
    from . import vignette as _vg

    vs = _vg.as_per_unit(vignette, 2)
    for im in (left, right):
        _vg.check_dtype(im.dtype)
    if auto_radius_on_device:
        raise NotImplementedError("vignette: with auto_radius_on_device=True the radius never reaches the host, where the gain's geometry "
                                  "is made; pass auto_radius_on_device=None (the exact form) or a numeric radius")
    fits = None
    if isinstance(center, str):
        fits = None if _capturing() else fit_circles([left, right])
        center = fit_centers(center, [left, right], fits=fits)
    elif isinstance(radius, str) and radius == "fit":
        fits = fit_circles([left, right])
    centers = per_unit_centers(center, 2)
    if isinstance(radius, str) and radius == "auto":
        _TLS.auto_form = "exact"
    if isinstance(transformer, tuple):  # per-eye transformer AND per-eye radius (remapper.py:460-473)
        r = [get_radius_smart(radius, [im]) if fits is None else get_radius_smart(radius, [im], fits=[f])
             for im, f in zip((left, right), fits or (None, None))]
    else:
        r = [get_radius_smart(radius, [left, right]) if fits is None else get_radius_smart(radius, [left, right], fits=fits)] * 2
    eyes = [_vg.correct_sources([im], v, centers=None if centers is None else [centers[k]], radius=r[k], inplace=inplace[k])[0]
            for k, (im, v) in enumerate(zip((left, right), vs))]
    return eyes[0], eyes[1], (r[0] if r[0] == r[1] else (r[0], r[1])), center


def _check_match_colors(match_colors: Any, match_reference: Any, left: Any, right: Any) -> None:
    """the arguments of ``match_colors=``, before anything is remapped"""
    if match_colors not in ("gain", "histogram"):
        raise ValueError(f'match_colors must be None, "gain" or "histogram", not {match_colors!r}')
    if match_reference not in ("left", "right"):
        raise ValueError(f'match_reference must be "left" or "right", not {match_reference!r}')
    for im in (left, right):
        if str(im.dtype).replace("torch.", "") != "uint8":
            raise ValueError(f"match_colors: uint8 images only, not {im.dtype} (wide pixels need a histogram of their own design)")


def anaglyph_tensors(left: torch.Tensor, right: torch.Tensor) -> torch.Tensor:
    """``merge=True`` of apply_lr on the device (reference remapper.py:485-497): per-eye channel
    mean times a colour, summed, / 255 -- a float64 ``(H, W, 3)`` tensor like the reference's
    ``combine`` (the "L" / "R" labels of :498-516 are not drawn here).  Current stream, no sync."""
    _check_image_tensor(left, "left")
    _check_image_tensor(right, "right")
    if left.dtype != torch.uint8 or right.dtype != torch.uint8:  # (the kernel reads bytes; apply_lr does wide types on the host)
        raise TypeError(f"anaglyph_tensors: uint8 images only, not {left.dtype} / {right.dtype}")
    if left.shape != right.shape or left.shape[2] != 3 or left.device != right.device:
        raise ValueError("anaglyph needs two (H, W, 3) uint8 tensors of the same shape on one device")
    h, w = int(left.shape[0]), int(left.shape[1])
    out = torch.empty((h, w, 3), dtype=torch.float64, device=left.device)
    rc = _native.lib().v1c_anaglyph(left.device.index, _stream_ptr(left.device), left.data_ptr(), left.stride(0),
                                    right.data_ptr(), right.stride(0), h, w, out.data_ptr(), out.stride(0) * 8)
    _native.check(rc, "v1c_anaglyph")
    return out


def apply_lr(
    transformer: TransformerBase | tuple[TransformerBase, TransformerBase],
    *,
    left_path: Path | str | NDArray,
    right_path: Path | str | NDArray,
    out_path: Path | str | None,
    size_output: tuple[int, int] = (2048, 2048),
    interpolation: int = INTER_LANCZOS4,
    boarder_mode: int = BORDER_CONSTANT,
    boarder_value: int | tuple[int, int, int] = 0,
    radius: float | Literal["auto", "max"] = "auto",
    merge: bool = False,
    device: Any = None,
    device_png: bool = False,
    device_jpeg: bool | Literal["batch", "vr180"] = False,
    device_decode: bool | Literal["batch"] = False,
    device_jpeg_optimize: bool = False,
    device_decode_progressive: bool = False,
    center: Any = None,
    match_colors: Literal["gain", "histogram"] | None = None,
    match_reference: Literal["left", "right"] = "left",
    chromatic: Any = None,
    vignette: Any = None,
) -> None:
    """Apply transformer to a pair of images and save them side by side (reference
    remapper.py:406-520).  ``left_path == right_path`` means one file holding both eyes.

    ``device_png=True``: a ``.png`` ``out_path`` of a uint8 / uint16 side-by-side result is deflated on the device
    (png_device.imwrite_tensor) and the raw result is not copied to the host; ``merge=True`` and other formats take the host route.
    ``device_jpeg=True``: the same for a ``.jpg`` / ``.jpeg`` ``out_path`` of a uint8 result (jpeg_device.imwrite_jpeg_tensor:
    quality 95, 4:2:0, as the host writer).  ``device_jpeg="batch"``: accepted as in ``apply``; the side-by-side frame is a batch of
    one (jpeg_device.imwrite_jpeg_tensors), the same bytes.  ``device_jpeg_optimize=True``: with either mode, the file gets Huffman
    tables built for the image on the device (``optimize=True`` of jpeg_device.py).  ``device_jpeg="vr180"``: the result is written as a
    Google VR180 photo instead of a side-by-side frame -- the two halves are encoded on the device as a batch of two and the right eye
    is embedded in the left eye's XMP (vr180_photo.imwrite_vr180_tensor); ``ValueError`` with ``merge=True`` or for a result the
    device encoder does not take.
    ``device_decode=True``: ``.jpg`` / ``.jpeg`` inputs are decoded on the device (jpeg_decode_device.py) and only their bytes are
    uploaded; one file holding both eyes is decoded once and the halves are views of it.  Files outside the device decoder's scope
    are read by the host as before.  ``device_decode="batch"``: the same, with the two files decoded as one batch of two.
    ``device_decode_progressive=True``: with either mode, progressive JPEG inputs are decoded on the device too instead of going to the
    host reader (``progressive=True`` of jpeg_decode_device.py).
    ``center``: as in ``apply_lr_tensors`` -- ``(cx, cy)``, a pair of them per eye, or ``"auto"``.  With one file holding both eyes the
    centres are in each HALF's own coordinates, and ``"auto"`` fits each half: the circles of a side-by-side fisheye frame are nowhere
    near ``W // 2`` of their halves.
    ``match_colors``, ``match_reference``: as in ``apply_lr_tensors`` -- the colours of one remapped eye matched to the other's on the
    device, before the anaglyph of ``merge=True`` and before every writer.  ValueError for a pair that is not uint8, before anything is
    remapped.  Where the result comes to the host anyway, a match that ended in a status (too few pixels in the mask) is logged as a
    warning; the device writers leave the report on the device.
    ``chromatic``: as in ``apply_lr_tensors`` -- a ``chromatic.ChromaticAberration`` or ``(left, right)``; the remap's result is what
    ``match_colors``, ``merge`` and every writer then see.
    ``vignette``: as in ``apply_lr_tensors`` -- a ``vignette.Vignette`` or ``(left, right)``: the lens's radial gain on each eye in front
    of the remap.  Arrays and tensors of the caller's stay as they are; eyes this call read or decoded itself are corrected where they
    lie."""
    vr180 = isinstance(device_jpeg, str) and device_jpeg == "vr180"
    device_jpeg = True if vr180 else _device_jpeg_mode(device_jpeg)
    if vr180 and merge:
        raise ValueError('device_jpeg="vr180" writes the two eyes: it does not go with merge=True')
    if vr180 and not (isinstance(out_path, (str, Path)) and Path(out_path).suffix.lower() in (".jpg", ".jpeg")):
        raise ValueError(f'device_jpeg="vr180" takes a .jpg / .jpeg out_path, not {out_path}')  # (before anything is read or remapped)
    jpeg_kw = {"optimize": True} if device_jpeg_optimize else {}
    caller_left, caller_right = left_path, right_path
    if device_decode:
        if isinstance(left_path, (str, Path)) and isinstance(right_path, (str, Path)) and left_path == right_path:
            both = _decode_on_device([left_path], device, device_decode, device_decode_progressive)[0]
            if isinstance(both, torch.Tensor):
                left_path, right_path = both[:, : both.shape[1] // 2], both[:, both.shape[1] // 2 :]
        else:
            left_path, right_path = _decode_on_device([left_path, right_path], device, device_decode, device_decode_progressive)
    if isinstance(left_path, (str, Path)) and isinstance(right_path, (str, Path)) and left_path == right_path:
        image = _io.imread(left_path)
        left_path = image[:, : image.shape[1] // 2]
        right_path = image[:, image.shape[1] // 2 :]
    left, right = _io.imread_many([left_path, right_path])  # (two files: decoded side by side, the codecs release the GIL)
    ca_kw: dict = {}
    if chromatic is not None:  # (refused before the device is looked at)
        from . import chromatic as _ca

        _ca.as_per_unit(chromatic, 2)
        _ca.check_images([left, right])
        ca_kw = {"chromatic": chromatic}
    if vignette is not None:  # (likewise)
        from . import vignette as _vg

        _vg.as_per_unit(vignette, 2)
        for im in (left, right):
            _vg.check_dtype(im.dtype)
    on_device = isinstance(left, torch.Tensor) and left.is_cuda
    dev = left.device if on_device else _device(device)
    if match_colors is not None:
        _check_match_colors(match_colors, match_reference, left, right)
    lt, rt = _to_device(left, dev), _to_device(right, dev)
    # "auto" radius: estimated on the host images when they are numpy (one row each)
    radius_ = _radius_for_pair(radius, transformer, left, right)
    if vignette is not None:  # (in place where the eye is this call's own: an upload, or a decode the caller never sees)
        own = [not isinstance(q, torch.Tensor) for q in (caller_left, caller_right)]
        lt, rt, radius_, center = _vignette_pair(transformer, lt, rt, vignette, radius=radius_, center=center, inplace=own)
    sbs = apply_lr_tensors(transformer, lt, rt, size_output=size_output, interpolation=interpolation,
                           boarder_mode=boarder_mode, boarder_value=boarder_value, radius=radius_, center=center, **ca_kw)
    match_report = _match_sbs_colors(sbs, size_output[0], match_colors, match_reference) if match_colors is not None else None
    if merge and sbs.dtype != torch.uint8:
        # 16-bit / float32: the reference's own NumPy expression (remapper.py:485-497) on the host copy (the anaglyph kernel is 8-bit)
        w = size_output[0]
        host = sbs.cpu().numpy()
        images = [host[:, :w], host[:, w:]]
        colors = [(0, 128, 255), (255, 128, 0)]
        combine = np.mean(images[0], axis=-1)[..., None] * np.array(colors[0]).reshape([1] * (images[0].ndim - 1) + [3]) + (
            np.mean(images[1], axis=-1)[..., None] * np.array(colors[1]).reshape([1] * (images[1].ndim - 1) + [3]))
        combine /= 255
        combine = _io.draw_anaglyph_labels(combine)
    elif merge:
        # red/cyan anaglyph of the two halves, on the device (remapper.py:485-497); the labels need
        # cv2.putText and are drawn on the host copy when cv2 is importable (:498-516)
        w = size_output[0]
        combine = _io.draw_anaglyph_labels(anaglyph_tensors(sbs[:, :w], sbs[:, w:]).cpu().numpy())
    else:
        if device_png and out_path is not None and not vr180:
            from . import png_device

            if png_device.eligible(out_path, sbs):
                png_device.imwrite_tensor(out_path, sbs)
                LOG.info(f"Saved to {Path(out_path).absolute()}")
                return
        if device_jpeg and out_path is not None:
            from . import jpeg_device

            if vr180 and not jpeg_device.eligible(out_path, sbs):
                raise ValueError(f'device_jpeg="vr180" takes a .jpg / .jpeg out_path and a uint8 result, not {out_path} and {sbs.dtype}')
            if jpeg_device.eligible(out_path, sbs):
                if vr180:
                    from . import vr180_photo

                    vr180_photo.imwrite_vr180_tensor(out_path, sbs, **jpeg_kw)
                elif device_jpeg == "batch":
                    jpeg_device.imwrite_jpeg_tensors([out_path], [sbs], **jpeg_kw)
                else:
                    jpeg_device.imwrite_jpeg_tensor(out_path, sbs, **jpeg_kw)
                LOG.info(f"Saved to {Path(out_path).absolute()}")
                return
        combine = sbs.cpu().numpy()
    if match_report is not None:  # (the result is on the host: the report costs no further wait)
        from . import colormatch

        rep = colormatch.color_match_report(match_report)
        if rep.status:
            LOG.warning(f"match_colors: the eyes were left as they are: {colormatch.STATUS.get(rep.status, rep.status)} (n = {rep.n})")
    if out_path is not None:
        _io.imwrite(out_path, combine)
        LOG.info(f"Saved to {Path(out_path).absolute()}")


def _match_sbs_colors(sbs: torch.Tensor, w: int, mode: str, reference: str) -> torch.Tensor:
    """the halves of a side-by-side result matched in place (colormatch.py); returns the report record, left on the device"""
    from . import colormatch

    halves = (sbs[:, :w], sbs[:, w:])
    luts, report = colormatch.color_match_luts_tensor(*halves, mode=mode, reference=reference)
    target = halves[1] if reference == "left" else halves[0]
    colormatch.apply_luts_tensor(target, luts, out=target)
    return report


def _radius_for_pair(radius, transformer, left, right):
    """``radius`` argument to hand to apply_lr_tensors: estimate 'auto' on the host images when
    they are numpy (the reference's estimate, remapper.py:82-84), else let the device path do it."""
    if isinstance(radius, str) and radius == "auto" and not isinstance(left, torch.Tensor):
        if isinstance(transformer, tuple):
            r = [get_radius_smart("auto", [im]) for im in (left, right)]
            return r[0] if r[0] == r[1] else radius
        return get_radius_smart("auto", [left, right])
    return radius


def __getattr__(name: str):
    # rotation_match / rotation_match_robust / match_lr live in vr180_convert.remapper in the
    # reference (remapper.py:93-321); here they are in calibration.py (which imports this module)
    if name in ("rotation_match", "rotation_match_robust", "match_lr", "calibration_rotators"):
        from . import calibration

        return getattr(calibration, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
