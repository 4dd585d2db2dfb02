"""ctypes binding of the HIP engine (``csrc/libvr180remap.so``, C ABI in include/vr180_remap.h).

There is no CPU fallback: if the library is missing, every image entry point raises.
Build it with ``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C
vr180_convert_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

from . import _abi

import os

# V1C_LIB: alternative build of the same ABI (kernel-tuning experiments); default = the in-tree build
LIB_PATH = Path(os.environ.get("V1C_LIB") or (Path(__file__).resolve().parent / "csrc" / "libvr180remap.so"))

SYMBOLS = [
    "v1c_abi_version", "v1c_device_count", "v1c_last_error", "v1c_plan_create", "v1c_plan_destroy",
    "v1c_plan_path", "v1c_plan_run", "v1c_plan_get_map", "v1c_remap_fused", "v1c_remap_lut",
    "v1c_get_radius", "v1c_get_radius_async", "v1c_build_itab", "v1c_anaglyph", "v1c_fused_cache_size", "v1c_plan_last_launch",
    "v1c_plan_release_captures", "v1c_plan_run_auto", "v1c_plan_run_auto_images",
    "v1c_plan_create_ex", "v1c_remap_lut_ex", "v1c_build_ftab",
    "v1c_feat_detect", "v1c_feat_match", "v1c_feat_pattern",
    "v1c_png_bound", "v1c_png_deflate",
    "v1c_jpeg_bound", "v1c_jpeg_header", "v1c_jpeg_encode", "v1c_jpeg_encode_batch",
    "v1c_jpeg_decode_info", "v1c_jpeg_decode", "v1c_jpeg_decode_batch",
    "v1c_jpeg_header_opt", "v1c_jpeg_encode_opt", "v1c_jpeg_encode_batch_opt",
    "v1c_jpeg_prog_info", "v1c_jpeg_prog_decode",
    "v1c_jpeg_transcode_bound", "v1c_jpeg_transcode_check", "v1c_jpeg_header_xc", "v1c_jpeg_transcode",
    "v1c_jpeg_compose_bound", "v1c_jpeg_compose_check", "v1c_jpeg_header_xf", "v1c_jpeg_compose",
    "v1c_fit_circle_workspace", "v1c_fit_circle_async", "v1c_fit_circle",
    "v1c_color_match_workspace", "v1c_color_match_luts_async", "v1c_apply_luts_async",
    "v1c_plan_tap_table_bytes", "v1c_plan_tap_entry_bytes",
    "v1c_ca_plan_create", "v1c_ca_plan_run", "v1c_ca_plan_get_map", "v1c_ca_plan_path", "v1c_ca_plan_last_launch", "v1c_ca_plan_destroy",
    "v1c_vignette_apply_async", "v1c_vignette_rings_async",
]


class EngineUnavailable(RuntimeError):
    """The HIP library is not built / not loadable."""


class EngineError(RuntimeError):
    """A C-ABI call returned an error code."""


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise EngineUnavailable(
            f"{LIB_PATH} is missing: build the HIP engine first (make -C {LIB_PATH.parent}); "
            "vr180_convert_amd has no CPU fallback"
        )
    try:
        L = C.CDLL(str(LIB_PATH))
    except OSError as e:  # pragma: no cover - depends on the machine
        raise EngineUnavailable(f"cannot load {LIB_PATH}: {e}") from e
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.v1c_abi_version.restype = i32
    L.v1c_device_count.restype = i32
    L.v1c_last_error.restype = C.c_char_p
    L.v1c_plan_create.argtypes = [C.POINTER(vp), i32, C.POINTER(_abi.Chain), i32, i32, i32, i32, i32, i32, i32, vp]
    L.v1c_plan_destroy.argtypes = [vp]
    L.v1c_plan_path.argtypes = [vp]
    L.v1c_plan_last_launch.argtypes = [vp]
    L.v1c_plan_last_launch.restype = i32
    try:
        L.v1c_plan_release_captures.argtypes = [vp]
        L.v1c_plan_run_auto.argtypes = [vp, vp, C.POINTER(_abi.Unit), i32, vp, i32]
        L.v1c_plan_run_auto_images.argtypes = [vp, vp, C.POINTER(_abi.Unit), i32, i32]
    except AttributeError:  # (an older build behind V1C_LIB: A/B runs of tools/ab.sh only)
        pass
    try:
        L.v1c_plan_create_ex.argtypes = [C.POINTER(vp), i32, C.POINTER(_abi.Chain), i32, i32, i32, i32, i32, i32, i32, i32, vp]
        L.v1c_remap_lut_ex.argtypes = [i32, vp, vp, i32, i32, i64, i32, i32, vp, i32, i32, i64, vp, vp, i64, i32, i32, vp]
        L.v1c_build_ftab.argtypes = [i32, vp]
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    try:
        L.v1c_feat_detect.argtypes = [i32, vp, vp, i32, i32, i64, i32, vp, vp, vp, vp]
        L.v1c_feat_match.argtypes = [i32, vp, vp, i32, vp, i32, vp, vp, vp, vp]
        L.v1c_feat_pattern.argtypes = [vp]
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    try:
        L.v1c_png_bound.argtypes = [i32, i32, i32, i32, i32]
        L.v1c_png_bound.restype = C.c_uint64
        L.v1c_png_deflate.argtypes = [i32, vp, vp, i32, i32, i64, i32, i32, i32, i32, vp, C.c_uint64, vp, vp, vp]
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    try:
        L.v1c_jpeg_bound.argtypes = [i32, i32, i32, i32, i32]
        L.v1c_jpeg_bound.restype = C.c_uint64
        L.v1c_jpeg_header.argtypes = [i32, i32, i32, i32, i32, i32, vp, C.c_uint64]
        L.v1c_jpeg_header.restype = i64
        L.v1c_jpeg_encode.argtypes = [i32, vp, vp, i32, i32, i64, i32, i32, i32, i32, vp, C.c_uint64, vp]
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    try:
        L.v1c_jpeg_decode_info.argtypes = [C.c_char_p, C.c_uint64, vp]
        L.v1c_jpeg_decode.argtypes = [i32, vp, C.c_char_p, C.c_uint64, vp, i64, i32, C.c_uint32, vp]
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    try:
        L.v1c_jpeg_decode_batch.argtypes = [i32, vp, i32, vp, vp, vp, vp, vp, C.c_uint32, C.c_uint64, vp, vp, vp]
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    try:
        L.v1c_jpeg_encode_batch.argtypes = [i32, vp, i32, vp, C.c_uint64, vp]
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    try:
        L.v1c_jpeg_header_opt.argtypes = [i32, i32, i32, i32, i32, i32, vp, C.c_uint32, vp, C.c_uint64]
        L.v1c_jpeg_header_opt.restype = i64
        L.v1c_jpeg_encode_opt.argtypes = [i32, vp, vp, i32, i32, i64, i32, i32, i32, i32, vp, C.c_uint64, vp, vp, vp]
        L.v1c_jpeg_encode_batch_opt.argtypes = [i32, vp, i32, vp, C.c_uint64, vp]
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    try:
        L.v1c_jpeg_prog_info.argtypes = [C.c_char_p, C.c_uint64, vp]
        L.v1c_jpeg_prog_decode.argtypes = [i32, vp, C.c_char_p, C.c_uint64, vp, i64, i32, C.c_uint32, vp, vp, C.c_uint32]
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    try:
        L.v1c_jpeg_transcode_bound.argtypes = [C.c_char_p, C.c_uint64, i32, i32, i32]
        L.v1c_jpeg_transcode_bound.restype = C.c_uint64
        L.v1c_jpeg_transcode_check.argtypes = [C.c_char_p, C.c_uint64, i32, vp, vp]
        L.v1c_jpeg_header_xc.argtypes = [C.c_char_p, C.c_uint64, i32, i32, i32, vp, C.c_uint32, vp, C.c_uint64]
        L.v1c_jpeg_header_xc.restype = i64
        L.v1c_jpeg_transcode.argtypes = [i32, vp, C.c_char_p, C.c_uint64, i32, vp, C.c_uint32, vp]
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    try:
        L.v1c_jpeg_compose_bound.argtypes = [C.c_char_p, C.c_uint64, i32, i32, i32]
        L.v1c_jpeg_compose_bound.restype = C.c_uint64
        L.v1c_jpeg_compose_check.argtypes = [i32, vp, i32, vp, vp]
        L.v1c_jpeg_header_xf.argtypes = [C.c_char_p, C.c_uint64, i32, i32, i32, i32, vp, C.c_uint32, vp, C.c_uint64]
        L.v1c_jpeg_header_xf.restype = i64
        L.v1c_jpeg_compose.argtypes = [i32, vp, i32, vp, i32, vp, C.c_uint32, vp]
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    try:
        L.v1c_fit_circle_workspace.argtypes = [i32, i32]
        L.v1c_fit_circle_workspace.restype = C.c_uint64
        L.v1c_fit_circle_async.argtypes = [i32, vp, vp, i32, i32, i64, i32, i32, vp, vp, vp]
        L.v1c_fit_circle.argtypes = [i32, vp, vp, i32, i32, i64, i32, i32, vp, vp, vp, vp, i32, vp]
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    try:
        L.v1c_color_match_workspace.argtypes = []
        L.v1c_color_match_workspace.restype = C.c_uint64
        L.v1c_color_match_luts_async.argtypes = [i32, vp, vp, i64, vp, i64, i32, i32, i32, vp, vp, vp, vp]
        L.v1c_apply_luts_async.argtypes = [i32, vp, vp, i64, vp, i64, i32, i32, i32, vp]
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    try:
        L.v1c_ca_plan_create.argtypes = [C.POINTER(vp), i32, C.POINTER(_abi.Chain), i32, i32, i32, i32, i32, i32, vp]
        L.v1c_ca_plan_run.argtypes = [vp, vp, C.POINTER(_abi.Unit), i32]
        L.v1c_ca_plan_get_map.argtypes = [vp, vp, i32, vp, vp, i64, vp]
        L.v1c_ca_plan_path.argtypes = [vp]
        L.v1c_ca_plan_last_launch.argtypes = [vp]
        L.v1c_ca_plan_destroy.argtypes = [vp]
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    try:
        L.v1c_vignette_apply_async.argtypes = [i32, vp, vp, i64, vp, i64, i32, i32, i32, i32, vp, vp]
        L.v1c_vignette_rings_async.argtypes = [i32, vp, vp, i64, i32, i32, i32, i32, vp, vp]
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    try:
        L.v1c_plan_tap_table_bytes.argtypes = [vp]
        L.v1c_plan_tap_table_bytes.restype = i64
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    try:
        L.v1c_plan_tap_entry_bytes.argtypes = [vp]
        L.v1c_plan_tap_entry_bytes.restype = i32
    except AttributeError:  # (an older build behind V1C_LIB)
        pass
    L.v1c_plan_run.argtypes = [vp, vp, C.POINTER(_abi.Unit), i32]
    L.v1c_plan_get_map.argtypes = [vp, vp, vp, vp, i64, vp]
    L.v1c_remap_fused.argtypes = [i32, vp, vp, i32, i32, i64, i32, vp, i32, i32, i64, C.POINTER(_abi.Chain), i32, i32, vp]
    L.v1c_remap_lut.argtypes = [i32, vp, vp, i32, i32, i64, i32, vp, i32, i32, i64, vp, vp, i64, i32, i32, vp]
    L.v1c_get_radius.argtypes = [i32, vp, vp, i32, i32, i64, i32, i32, C.POINTER(C.c_double)]
    L.v1c_get_radius_async.argtypes = [i32, vp, vp, i32, i32, i64, i32, i32, vp]
    L.v1c_fused_cache_size.restype = i32
    L.v1c_build_itab.argtypes = [i32, vp]
    L.v1c_anaglyph.argtypes = [i32, vp, vp, i64, vp, i64, i32, i32, vp, i64]
    if L.v1c_abi_version() != _abi.ABI_VERSION:
        raise EngineUnavailable("libvr180remap.so was built for a different ABI version; rebuild it")
    _lib = L
    return L


def check(rc: int, what: str) -> None:
    """Raise the Python exception matching a non-zero return code."""
    if rc == _abi.OK:
        return
    msg = lib().v1c_last_error().decode("utf-8", "replace")
    if rc == _abi.E_INVALID:
        raise ValueError(f"{what}: {msg}")
    if rc == _abi.E_UNSUPPORTED:
        raise NotImplementedError(f"{what}: {msg}")
    raise EngineError(f"{what}: {msg} (code {rc})")
