"""MI355X-native drop-in for the hot path of 34j/vr180-convert: ``apply`` / ``apply_lr`` /
``get_map`` and the Transformer classes (reference src/vr180_convert/__init__.py:1-32)."""
__version__ = "0.1.0"

from .chain import (
    DenormalizeTransformer,
    EquirectangularEncoder,
    Euclidean3DRotator,
    Euclidean3DTransformer,
    FisheyeDecoder,
    FisheyeEncoder,
    MultiTransformer,
    NormalizeTransformer,
    PolarRollTransformer,
    TransformerBase,
    ZoomTransformer,
)
from .remapper import (anaglyph_tensors, apply, apply_lr, apply_lr_tensors, auto_radius_tensor, get_map, remap_tensors,
                       remap_tensors_auto)
from .features import detect, match, match_points_device
from .png_device import encode_png_tensor, imwrite_tensor
from .jpeg_device import (encode_jpeg_tensor, encode_jpeg_tensors, imwrite_jpeg_tensor, imwrite_jpeg_tensors,
                          last_encode_batch_report)
from .jpeg_decode_device import (decode_jpeg_tensor, decode_jpeg_tensors, imread_tensor, imread_tensors, last_batch_report,
                                 last_decode_report)
from .jpeg_transcode_device import split_sbs_jpeg, swap_sbs_jpeg, transcode_jpeg
from .jpeg_compose_device import (compose_regions, join_sbs_jpeg, normalize_orientation_jpeg, sbs_from_vr180_photo,
                                  transform_jpeg)
from .sharding import remap_sharded
from .circle import Circle, fit_circle, fit_circle_tensor

_VIGNETTE = ("Vignette", "gain_tables", "apply_vignette_tensor", "vignette_rings_tensor", "fit_vignette")
_COLORMATCH = ("color_match_luts_tensor", "apply_luts_tensor", "match_eyes_tensors", "color_match_report", "ColorMatchReport")


def __getattr__(name: str):
    # colormatch.py is imported on first use: an apply_lr without match_colors= runs none of it
    if name in _COLORMATCH:
        from . import colormatch

        return getattr(colormatch, name)
    if name == "ChromaticAberration":  # (likewise: a remap without chromatic= imports none of chromatic.py)
        from . import chromatic

        return chromatic.ChromaticAberration
    if name in _VIGNETTE:  # (and a remap without vignette= imports none of vignette.py)
        from . import vignette

        return getattr(vignette, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = [
    "TransformerBase",
    "ZoomTransformer",
    "MultiTransformer",
    "NormalizeTransformer",
    "PolarRollTransformer",
    "DenormalizeTransformer",
    "FisheyeDecoder",
    "FisheyeEncoder",
    "EquirectangularEncoder",
    "Euclidean3DRotator",
    "Euclidean3DTransformer",
    "apply",
    "apply_lr",
    "get_map",
    # additions of this engine (device-resident entry points)
    "apply_lr_tensors",
    "anaglyph_tensors",
    "remap_tensors",
    "remap_tensors_auto",
    "auto_radius_tensor",
    "remap_sharded",
    # feature matching of the two eyes (--automatch devfm)
    "detect",
    "match",
    "match_points_device",
    # PNG files of device-resident results, deflated on the device (device_png=True / --device-png)
    "encode_png_tensor",
    "imwrite_tensor",
    # JPEG files of device-resident results, encoded on the device (device_jpeg=True / --device-jpeg)
    "encode_jpeg_tensor",
    "imwrite_jpeg_tensor",
    # ... a list of them in shared launches (device_jpeg="batch" / --device-jpeg-batch)
    "encode_jpeg_tensors",
    "imwrite_jpeg_tensors",
    "last_encode_batch_report",
    # JPEG inputs decoded on the device into tensors (device_decode=True / --device-decode)
    "decode_jpeg_tensor",
    "imread_tensor",
    "last_decode_report",
    # ... a list of them in shared launches and rounds (device_decode="batch" / --device-decode-batch)
    "decode_jpeg_tensors",
    "imread_tensors",
    "last_batch_report",
    # lossless crop, split and swap of JPEG files in the DCT domain, on the device (swap --lossless, xmp --device)
    "transcode_jpeg",
    "split_sbs_jpeg",
    "swap_sbs_jpeg",
    # lossless join, rotation and flip of JPEG files in the DCT domain, from several files, on the device (join)
    "compose_regions",
    "transform_jpeg",
    "join_sbs_jpeg",
    "sbs_from_vr180_photo",
    "normalize_orientation_jpeg",
    # centre and radius of the image circle from its rim, fitted on the device (center="auto", radius="fit")
    "fit_circle",
    "fit_circle_tensor",
    "Circle",
    # the colours of one eye matched to the other's on the device (match_colors= / --match-colors)
    "color_match_luts_tensor",
    "apply_luts_tensor",
    "match_eyes_tensors",
    "color_match_report",
    "ColorMatchReport",
    # lateral chromatic aberration corrected inside the remap, one map per colour channel (chromatic= / --chromatic)
    "ChromaticAberration",
    # lens vignetting corrected by a radial gain in front of the remap, and fitted from a flat-field frame (vignette= / --vignette)
    "Vignette",
    "gain_tables",
    "apply_vignette_tensor",
    "vignette_rings_tensor",
    "fit_vignette",
]
