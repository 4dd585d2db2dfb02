"""Lateral chromatic aberration: one remap map per colour channel of a BGR image.

A fisheye lens magnifies red, green and blue by slightly different amounts; at the rim of the image circle the channels can be one to
three source pixels apart.  The correction is a radial rescaling of the source position per channel, so it is part of the remap:
``ChromaticAberration(red=coefs, blue=coefs)`` appends a ``PolynomialScaler`` to the transformer chain of that channel, directly in
front of the ``DenormalizeTransformer`` ``get_map`` appends, and the engine remaps the three channels in one launch
(``v1c_ca_plan_*``, csrc/chroma.hip).  Channel ``c`` of the result is, byte for byte, channel ``c`` of what the plain entry point gives
for ``transformer * PolynomialScaler(coefs_c)``.

``remap_tensors``, ``apply``, ``apply_lr``, ``apply_lr_tensors`` and ``get_map`` (remapper.py) take it as ``chromatic=``.
"""
from __future__ import annotations

import ctypes as C
import threading
import time
from collections import OrderedDict
from dataclasses import dataclass
from typing import Any, Sequence

import numpy as np

from . import _abi, _native
from .chain import NotLowerable, PolynomialScaler, TransformerBase, lower_for_get_map

CHANNELS = ("b", "g", "r")  # the order of a BGR pixel's bytes, and of the chains a plan takes


def _coefs(v: Any, what: str) -> tuple[float, ...] | None:
    if v is None:
        return None
    try:
        out = tuple(float(c) for c in v)
    except (TypeError, ValueError):
        raise ValueError(f"ChromaticAberration({what}=...): a sequence of numbers (PolynomialScaler.coefs_reverse) or None") from None
    if not out or len(out) > _abi.MAX_PARAMS or not all(np.isfinite(out)):
        raise ValueError(f"ChromaticAberration({what}=...): 1 to {_abi.MAX_PARAMS} finite coefficients")
    return out


@dataclass(frozen=True)
class ChromaticAberration:
    """Per-channel radial polynomials.  Each is a ``PolynomialScaler.coefs_reverse`` -- lowest order first -- in units of the
    image-circle radius: the stage sees the normalised source position, 1.0 is the rim, and returns where that channel is read.
    ``None`` or ``[0, 1]`` (the identity) appends nothing: the channel keeps the plain chain and its table.  Green is usually the
    reference channel and left alone."""

    red: Sequence[float] | None = None
    blue: Sequence[float] | None = None
    green: Sequence[float] | None = None

    def __post_init__(self):
        for name in ("red", "blue", "green"):
            object.__setattr__(self, name, _coefs(getattr(self, name), name))

    def coefs(self, channel: str) -> tuple[float, ...] | None:
        """the coefficients appended for channel 'b' / 'g' / 'r'; None: nothing is appended"""
        c = {"b": self.blue, "g": self.green, "r": self.red}[channel]
        return None if c is None or c == (0.0, 1.0) else c

    def key(self) -> tuple:
        """exact, hashable: equal objects share it, any other coefficient does not (floats by their bits)"""
        return tuple(None if self.coefs(ch) is None else tuple(v.hex() for v in self.coefs(ch)) for ch in CHANNELS)

    def channel_transformers(self, transformer: TransformerBase) -> tuple[TransformerBase, TransformerBase, TransformerBase]:
        """``(t_B, t_G, t_R)``: ``transformer * PolynomialScaler(coefs_c)`` -- the stage lands last -- or ``transformer`` itself"""
        return tuple(transformer if self.coefs(ch) is None else transformer * PolynomialScaler(coefs_reverse=list(self.coefs(ch))) for ch in CHANNELS)


def parse(text: str) -> ChromaticAberration:
    """``"r:0,1.0012,0,-0.0009;b:0,0.9991,0,0.0006"`` -> ChromaticAberration (the CLI's ``--chromatic``); ValueError with a reason"""
    if not isinstance(text, str) or not text.strip():
        raise ValueError("empty chromatic specification")
    got: dict[str, list[float]] = {}
    for part in text.split(";"):
        if not part.strip():
            continue
        name, sep, vals = part.partition(":")
        name = name.strip().lower()
        if not sep or name not in ("r", "g", "b"):
            raise ValueError(f"{part.strip()!r}: expected CHANNEL:c0,c1,... with CHANNEL one of r, g, b")
        if name in got:
            raise ValueError(f"channel {name!r} given twice")
        try:
            got[name] = [float(v) for v in vals.split(",")]
        except ValueError:
            raise ValueError(f"{part.strip()!r}: coefficients must be numbers separated by commas") from None
    if not got:
        raise ValueError("empty chromatic specification")
    return ChromaticAberration(red=got.get("r"), blue=got.get("b"), green=got.get("g"))


def parse_pair(text: str) -> "ChromaticAberration | tuple[ChromaticAberration, ChromaticAberration]":
    """``--chromatic`` of the pair commands: one specification for both eyes, or ``LEFT|RIGHT``"""
    if "|" in text:
        parts = text.split("|")
        if len(parts) != 2:
            raise ValueError("expected LEFT|RIGHT: one '|' between the two eyes' specifications")
        return parse(parts[0]), parse(parts[1])
    return parse(text)


def as_per_unit(chromatic: Any, n: int) -> list[ChromaticAberration]:
    """``chromatic=`` of a call with ``n`` units: one object for all of them, or one per unit (the pair entries' ``(left, right)``)"""
    if isinstance(chromatic, ChromaticAberration):
        return [chromatic] * n
    if isinstance(chromatic, (tuple, list)) and len(chromatic) == n and all(isinstance(c, ChromaticAberration) for c in chromatic):
        return list(chromatic)
    raise TypeError(f"chromatic must be a ChromaticAberration or one per image ({n}), not {chromatic!r}")


def check_images(images: Sequence[Any]) -> None:
    """What the chromatic remap refuses, before anything touches the device: images that are not 3-channel (ValueError) or not uint8
    (TypeError).  ``images``: tensors or arrays."""
    for k, im in enumerate(images):
        dt = str(im.dtype).replace("torch.", "")
        if dt != "uint8":
            raise TypeError(f"chromatic: image {k} is {dt}; the per-channel remap takes uint8 images only")
        shape = tuple(im.shape)
        if len(shape) != 3 or shape[2] != 3:
            raise ValueError(f"chromatic: image {k} has shape {shape}; the per-channel remap takes 3-channel (BGR) images only")


def lower_channels(transformer: TransformerBase, chromatic: ChromaticAberration, *, radius: float, size_input, size_output,
                   center: Any = None) -> tuple[_abi.Chain, _abi.Chain, _abi.Chain]:
    """The three lowered chains (B, G, R) of one unit: radius, centre and sizes go into every channel chain the same way.
    NotImplementedError for a transformer that cannot be lowered (its map would have to come from its own NumPy ``transform``)."""
    out = []
    lowered: dict[int, _abi.Chain] = {}
    for t in chromatic.channel_transformers(transformer):
        if id(t) not in lowered:
            try:
                lowered[id(t)] = lower_for_get_map(t, radius=radius, size_input=size_input, size_output=size_output, center=center)
            except NotLowerable as e:
                raise NotImplementedError(f"chromatic: the transformer chain cannot be lowered ({e}); the per-channel remap has no "
                                          "host-map route") from None
        out.append(lowered[id(t)])
    return tuple(out)


def plan_key(chains: Sequence[_abi.Chain], *, src_hw, dst_wh, interpolation, border_mode, border_value, device_index) -> tuple:
    """the cache key of a CaPlan: the scheme of remapper._plan_for with three chains in place of one"""
    from .remapper import border_scalar

    return ("ca", tuple(ch.key() for ch in chains), tuple(src_hw), tuple(dst_wh), int(interpolation), int(border_mode),
            border_scalar(border_value).tobytes(), device_index)


class CaPlan:
    """Owner of one ``v1c_ca_plan`` (include/vr180_remap.h): three channel chains of one BGR remap."""

    cn = 3

    def __init__(self, chains: Sequence[_abi.Chain], *, src_hw, dst_wh, interpolation, border_mode, border_value, device):
        import torch

        from .remapper import _device, border_scalar

        self.device = _device(device)
        self.src_hw, self.dst_wh = tuple(src_hw), tuple(dst_wh)
        self.dtype = torch.uint8
        self._h = C.c_void_p()
        self._memo: "OrderedDict[tuple, Any]" = OrderedDict()
        arr = (_abi.Chain * 3)(*chains)
        bv = border_scalar(border_value)
        t0 = time.perf_counter()
        rc = _native.lib().v1c_ca_plan_create(C.byref(self._h), self.device.index, arr, src_hw[0], src_hw[1], dst_wh[1], dst_wh[0],
                                              int(interpolation), int(border_mode), bv.ctypes.data)
        _native.check(rc, "v1c_ca_plan_create")
        self.create_ms = (time.perf_counter() - t0) * 1e3

    @property
    def path(self) -> str:
        """'ray' (fused: one ray direction per pixel, a radial table per channel) or 'literal' (three fp64 interpreters)"""
        return "ray" if _native.lib().v1c_ca_plan_path(self._h) == 1 else "literal"

    def last_launch(self) -> str:
        """'chroma', with '+fixup' when a fix-up pass followed; '' before the first run"""
        k = _native.lib().v1c_ca_plan_last_launch(self._h)
        if k < 0:
            return ""
        return _abi.LAUNCH_NAMES.get(k & 0xFF, "?") + ("+fixup" if k & _abi.LAUNCH_FIXUP else "")

    def run(self, srcs, dsts, rots: Sequence[Any] | None = None) -> None:
        from .remapper import _stream_ptr, marshal_units

        n = len(srcs)
        if n == 0 or len(dsts) != n or (rots is not None and len(rots) != n):
            raise ValueError("srcs / dsts / rots lengths differ or are empty")
        sig = None
        if rots is None:  # (a steady stream of calls on the same buffers reuses the marshalled units, like Plan.run)
            sig = tuple((s.data_ptr(), s.stride(), s.shape, s.dtype, d.data_ptr(), d.stride(), d.shape, d.dtype) for s, d in zip(srcs, dsts))
        units = self._memo.get(sig) if sig is not None else None
        if units is None:
            units = marshal_units(srcs, dsts, rots, src_hw=self.src_hw, dst_wh=self.dst_wh, cn=3, device=self.device, dtype=self.dtype)
            if sig is not None:
                self._memo[sig] = units
                while len(self._memo) > 64:
                    try:
                        self._memo.popitem(last=False)
                    except KeyError:
                        break
        rc = _native.lib().v1c_ca_plan_run(self._h, _stream_ptr(self.device), units, n)
        _native.check(rc, "v1c_ca_plan_run")

    def run_units(self, units: Any, n: int) -> None:
        """Launch an already marshalled ``v1c_unit`` array (``remapper.marshal_units``) on the current stream."""
        from .remapper import _stream_ptr

        rc = _native.lib().v1c_ca_plan_run(self._h, _stream_ptr(self.device), units, int(n))
        _native.check(rc, "v1c_ca_plan_run")

    def get_map(self, channel: str, rot: Any = None):
        import torch

        from .remapper import _stream_ptr

        w, h = self.dst_wh
        xm = torch.empty((h, w), dtype=torch.float32, device=self.device)
        ym = torch.empty((h, w), dtype=torch.float32, device=self.device)
        r = None if rot is None else np.ascontiguousarray(np.asarray(rot, np.float64).reshape(9))
        rc = _native.lib().v1c_ca_plan_get_map(self._h, _stream_ptr(self.device), channel_index(channel), xm.data_ptr(), ym.data_ptr(),
                                               xm.stride(0) * 4, None if r is None else r.ctypes.data)
        _native.check(rc, "v1c_ca_plan_get_map")
        return xm, ym

    def __del__(self):
        try:
            if self._h:
                _native.lib().v1c_ca_plan_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass


def channel_index(channel: Any) -> int:
    if isinstance(channel, str) and channel.lower() in CHANNELS:
        return CHANNELS.index(channel.lower())
    raise ValueError(f'channel must be "b", "g" or "r", not {channel!r}')


_PLANS: "OrderedDict[tuple, CaPlan]" = OrderedDict()
_PLAN_CACHE_SIZE = 32
_PLANS_LOCK = threading.Lock()


def clear_caches() -> None:
    with _PLANS_LOCK:
        _PLANS.clear()


def plan_for(chains: Sequence[_abi.Chain], *, src_hw, dst_wh, interpolation, border_mode, border_value, device) -> CaPlan:
    from .remapper import _device

    dev = _device(device)
    key = plan_key(chains, src_hw=src_hw, dst_wh=dst_wh, interpolation=interpolation, border_mode=border_mode,
                   border_value=border_value, device_index=dev.index)
    with _PLANS_LOCK:
        plan = _PLANS.get(key)
        if plan is not None:
            _PLANS.move_to_end(key)
            return plan
    plan = CaPlan(chains, src_hw=src_hw, dst_wh=dst_wh, interpolation=interpolation, border_mode=border_mode,
                  border_value=border_value, device=dev)
    with _PLANS_LOCK:
        plan = _PLANS.setdefault(key, plan)
        _PLANS.move_to_end(key)
        while len(_PLANS) > _PLAN_CACHE_SIZE:
            _PLANS.popitem(last=False)
    return plan


class CaGroup:
    """units of one call that share a CaPlan (remapper.LaunchGroup with three chains)"""

    __slots__ = ("chains", "src_hw", "srcs", "dsts", "rots", "index")

    def __init__(self, chains, src_hw, srcs, dsts, rots, index):
        self.chains, self.src_hw, self.srcs, self.dsts, self.rots, self.index = chains, src_hw, srcs, dsts, rots, index


def group_units(transformer, srcs, dsts, chromatic, *, radius: float, size_input=None, centers=None, rotations=None) -> list[CaGroup]:
    """Host logic of a call, no device involved (remapper.group_units for three chains per unit): lower the channel chains of every unit
    and split the units into groups that share a plan -- the same three chains up to the matrix of a single rotate stage, the same
    source size.  ``rotations``: one rotation per unit replacing that of the chain's single Euclidean3DRotator."""
    from .remapper import _split_single_rotation

    n = len(srcs)
    per_unit = list(transformer) if isinstance(transformer, (list, tuple)) else [transformer] * n
    if len(per_unit) != n or len(dsts) != n:
        raise ValueError("need one transformer and one dst per src")
    if rotations is not None and (isinstance(transformer, (list, tuple)) or len(rotations) != n):
        raise ValueError("rotations= needs ONE transformer chain and one rotation / dst per src")
    cas = as_per_unit(chromatic, n)
    src_hw = (int(srcs[0].shape[0]), int(srcs[0].shape[1]))
    dst_wh = (int(dsts[0].shape[1]), int(dsts[0].shape[0]))
    acc: "OrderedDict[bytes, dict]" = OrderedDict()
    lowered: dict[Any, Any] = {}
    for k, (t, ca) in enumerate(zip(per_unit, cas)):
        size_in_k = tuple(size_input) if size_input is not None else (
            src_hw if not isinstance(transformer, (list, tuple)) else (int(srcs[k].shape[0]), int(srcs[k].shape[1])))
        c_k = None if centers is None else centers[k]
        lk = (id(t), ca.key(), size_in_k, c_k)
        if lk not in lowered:
            lowered[lk] = lower_channels(t, ca, radius=radius, size_input=size_in_k, size_output=dst_wh, center=c_k)
        full = lowered[lk]
        split = [_split_single_rotation(ch) for ch in full]
        if any((s[1] is None) != (split[0][1] is None) for s in split):  # (cannot happen: the channels share the transformer)
            raise ValueError("chromatic: the channel chains disagree about their rotation")
        rot = split[0][1]
        if rotations is not None:
            from .quat import as_rotation_matrix

            if rot is None:
                raise ValueError("rotations= needs a chain with exactly one Euclidean3DRotator")
            rot = np.asarray(as_rotation_matrix(rotations[k]), np.float64).reshape(9)
        shared = tuple(s[0] for s in split)
        key = b"".join(bytes(ch) for ch in shared) + repr(tuple(srcs[k].shape)).encode()
        g = acc.setdefault(key, {"shared": shared, "full": full, "src_hw": tuple(int(v) for v in srcs[k].shape[:2]),
                                 "srcs": [], "dsts": [], "rots": [], "index": []})
        g["srcs"].append(srcs[k])
        g["dsts"].append(dsts[k])
        g["rots"].append(rot)
        g["index"].append(k)
    groups = []
    for g in acc.values():
        r0 = g["rots"][0]
        uniform = rotations is None and (r0 is None or all(np.array_equal(r, r0) for r in g["rots"]))
        groups.append(CaGroup(g["full"] if uniform else g["shared"], g["src_hw"], g["srcs"], g["dsts"],
                              None if uniform else g["rots"], g["index"]))
    return groups


def remap_tensors_chromatic(transformer, srcs, dsts, chromatic, *, radius, interpolation, boarder_mode, boarder_value, size_input=None,
                            rotations=None, centers=None) -> tuple[list[str], list[CaPlan]]:
    """``remapper.remap_tensors`` with ``chromatic=``: returns the path per launch group and the plans that ran"""
    check_images(list(srcs) + list(dsts))
    dst_wh = (int(dsts[0].shape[1]), int(dsts[0].shape[0]))
    groups = group_units(transformer, srcs, dsts, chromatic, radius=radius, size_input=size_input, centers=centers, rotations=rotations)
    dev = srcs[0].device
    paths, plans = [], []
    for g in groups:
        plan = plan_for(g.chains, src_hw=g.src_hw, dst_wh=dst_wh, interpolation=interpolation, border_mode=boarder_mode,
                        border_value=boarder_value, device=dev)
        plan.run(g.srcs, g.dsts, g.rots)
        plans.append(plan)
        paths.append(plan.path)
    return paths, plans


def get_map_channel(transformer, chromatic: ChromaticAberration, channel: str, *, radius, size_input, size_output, device=None, center=None):
    """``remapper.get_map`` of one channel ('b' / 'g' / 'r') through the plan the remap itself uses: float32 ``xmap, ymap`` arrays"""
    channel_index(channel)
    if not isinstance(chromatic, ChromaticAberration):
        raise TypeError(f"chromatic must be a ChromaticAberration, not {chromatic!r}")
    chains = lower_channels(transformer, chromatic, radius=radius, size_input=size_input, size_output=size_output, center=center)
    plan = plan_for(chains, src_hw=(max(1, size_input[0]), max(1, size_input[1])), dst_wh=size_output, interpolation=_abi.INTER_LINEAR,
                    border_mode=_abi.BORDER_CONSTANT, border_value=0, device=device)
    xm, ym = plan.get_map(channel)
    return xm.cpu().numpy(), ym.cpu().numpy()
