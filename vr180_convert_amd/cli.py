"""Command line of the engine: ``lr`` / ``s`` / ``swap`` / ``xmp`` with the options, defaults and file-name
rules of the reference's typer app (reference cli.py:116-559; entry points ``vr180-convert`` / ``v1c``,
pyproject.toml:25-27), so that ``v1c lr left.jpg right.jpg --transformer "..."`` runs unchanged -- the remap
itself happens on the MI355X through ``apply`` / ``apply_lr``.

What is OpenCV or libxmp from end to end -- AKAZE feature matching (``--automatch fm[scale]``, cli.py:255-262, with ``--savematch``),
the point-picking window (``--automatch gui[n]``, cli.py:82-113) and the ``xmp`` command (cli.py:439-540) -- lives in
``calibration_cv.py`` behind lazy imports: with the library installed the options work as in the reference, without it they report
which package is missing (the GPU image of this engine ships neither); explicit points (``--automatch "x,y;x,y;..."``) need nothing,
and neither does ``--automatch devfm[scale]``: the engine's own feature matcher on the GPU (``features.py``; not AKAZE).
"""
from __future__ import annotations

import hashlib
import logging
import re
from datetime import datetime, timezone
from pathlib import Path
from typing import Any, List, Optional, Sequence

import numpy as np
import typer
from typing_extensions import Annotated

from . import _abi, _io
from . import quat as _quat
from . import transformer as _T
from .calibration import calibration_rotators, match_lr, rotation_match, rotation_match_robust
from .chain import MultiTransformer

LOG = logging.getLogger(__name__)
DEFAULT_EXTENSION = "png"  # cli.py:39

app = typer.Typer(help="Fisheye -> VR180 side-by-side equirectangular conversion on MI355X.")

_INTERPOLATIONS = {"nearest": _abi.INTER_NEAREST, "linear": _abi.INTER_LINEAR, "cubic": _abi.INTER_CUBIC,
                   "area": _abi.INTER_AREA, "lanczos4": _abi.INTER_LANCZOS4}
_BORDERS = {"constant": _abi.BORDER_CONSTANT, "replicate": _abi.BORDER_REPLICATE, "reflect": _abi.BORDER_REFLECT,
            "wrap": _abi.BORDER_WRAP, "reflect_101": _abi.BORDER_REFLECT_101, "transparent": _abi.BORDER_TRANSPARENT}


def _flag(value: str, table: dict, prefix: str, what: str) -> int:
    """``INTER_LANCZOS4`` / ``inter_lanczos4`` / ``lanczos4`` -> the cv2 enum value (cli.py:57-79, :376-377)."""
    key = value.strip().lower()
    key = key[len(prefix):] if key.startswith(prefix) else key
    if key not in table:
        raise typer.BadParameter(f"unknown {what} {value!r}; one of " + ", ".join(prefix.upper() + k.upper() for k in table))
    return table[key]


def _namespace() -> dict:
    """Names a ``--transformer`` expression may use: the reference evaluates it inside cli.py, i.e. with numpy as
    ``np``, everything numpy-quaternion exports and every transformer name in scope (cli.py:12,15,20,233)."""
    ns: dict[str, Any] = {"np": np}
    ns.update({k: getattr(_T, k) for k in dir(_T) if not k.startswith("_")})
    ns.update({k: getattr(_quat, k) for k in ("quaternion", "from_euler_angles", "from_rotation_vector", "as_rotation_matrix",
                                              "rotate_vectors", "as_quat_array")})
    return ns


def parse_transformer(code: str) -> Any:
    """The transformer of a command: the default chain for ``""`` (cli.py:231), else the evaluated expression."""
    if code == "":
        return _T.EquirectangularEncoder() * _T.FisheyeDecoder("equidistant")
    return eval(code, _namespace())  # noqa: S307 - the CLI contract: the option is Python source (cli.py:233)


def parse_size(size: str) -> tuple[int, int]:
    w, h = (int(v) for v in size.lower().split("x"))
    return w, h


def parse_radius(radius: str) -> Any:
    return radius if radius in ("auto", "max", "fit") else float(radius)


def parse_center(center: str, *, pair: bool = True, swap: bool = False) -> Any:
    """``--center``: '' -> None (the frame's centre), 'auto' -> 'auto' (fitted per image), 'X,Y' -> (x, y), and for a pair of eyes
    'LX,LY;RX,RY' -> ((lx, ly), (rx, ry)), which ``swap`` exchanges with the eyes"""
    if center == "":
        return None
    if center == "auto":
        return "auto"
    try:
        pts = [tuple(float(v) for v in part.split(",")) for part in center.split(";")]
        if not all(len(q) == 2 for q in pts) or len(pts) not in ((1, 2) if pair else (1,)):
            raise ValueError(center)
    except ValueError as e:
        raise typer.BadParameter(f"--center {center}: expected 'auto', 'X,Y'" + (" or 'LX,LY;RX,RY'" if pair else "")) from e
    if len(pts) == 1:
        return pts[0]
    return (pts[1], pts[0]) if swap else (pts[0], pts[1])


def parse_chromatic(text: str, *, pair: bool = True, swap: bool = False) -> Any:
    """``--chromatic``: '' -> None, 'r:c0,c1,...;b:c0,c1,...' -> a ChromaticAberration (channels r, g, b; each a PolynomialScaler's
    coefs_reverse, 1.0 = the rim of the image circle), and for a pair of eyes 'LEFT|RIGHT' -> one per eye, which ``swap`` exchanges with
    the eyes"""
    if text == "":
        return None
    from . import chromatic

    try:
        if not pair and "|" in text:
            raise ValueError("one image per map: no per-eye 'LEFT|RIGHT' form here")
        ca = chromatic.parse_pair(text) if pair else chromatic.parse(text)
    except ValueError as e:
        raise typer.BadParameter(f"--chromatic {text}: {e}") from e
    if isinstance(ca, tuple) and swap:
        return (ca[1], ca[0])
    return ca


def parse_vignette(text: str, gamma: float = 1.0, *, pair: bool = True, swap: bool = False) -> Any:
    """``--vignette``: '' -> None, 'k1,k2,k3' or 'b:k1,k2,k3;g:...;r:...' -> a Vignette (V = 1 + k1 rho^2 + k2 rho^4 + k3 rho^6, 1.0 = the
    rim of the image circle) with ``--vignette-gamma``, and for a pair of eyes 'LEFT|RIGHT' -> one per eye, which ``swap`` exchanges with
    the eyes"""
    if text == "":
        return None
    from . import vignette

    try:
        if not pair and "|" in text:
            raise ValueError("one correction for every image: no per-eye 'LEFT|RIGHT' form here")
        v = vignette.parse_pair(text, gamma) if pair else vignette.parse(text, gamma)
    except ValueError as e:
        raise typer.BadParameter(f"--vignette {text} (--vignette-gamma {gamma}): {e}") from e
    if isinstance(v, tuple) and swap:
        return (v[1], v[0])
    return v


def closest_in_time(directory: Path, anchor: Path, offset_s: float) -> Path:
    """The file under ``directory`` (recursively) with ``anchor``'s suffix whose modification time is closest to
    ``anchor``'s, shifted by ``offset_s`` seconds (cli.py:178-216)."""
    target = anchor.stat().st_mtime + offset_s
    found = [p for p in directory.rglob("*") if p != anchor and p.suffix == anchor.suffix and p.is_file()]
    if not found:
        raise ValueError(f"No time-matched image found under {directory}")
    return min(found, key=lambda p: abs(p.stat().st_mtime - target))


def resolve_pair(left: Path, right: Path, r_earlier_l: float) -> tuple[Path, Path]:
    """One of the two paths may be a directory: it is searched for the image taken at the same time as the other
    one, the right camera's clock being ``r_earlier_l`` seconds ahead."""
    if left.is_dir() and right.is_dir():
        raise ValueError("Both left and right paths must not be directories")
    if left.is_dir():
        return closest_in_time(left, right, -r_earlier_l), right
    if right.is_dir():
        return left, closest_in_time(right, left, r_earlier_l)
    return left, right


def unique_suffix(*options: Any) -> str:
    """``-xxxxxxxx``: eight hex digits of the SHA-256 of the options that shape the output (cli.py:334-352)."""
    return "-" + hashlib.sha256("".join(str(o) for o in options).encode("utf-8")).hexdigest()[:8]


def output_path(out_path: Path, left: Path, right: Path, tag: str) -> Path:
    name = f"{left.stem}-{right.stem}{tag}.{DEFAULT_EXTENSION}"
    if out_path == Path(""):
        return left.parent / name
    return out_path / name if out_path.is_dir() else out_path


def split_at_first_encoder(t: Any) -> tuple[MultiTransformer, MultiTransformer]:
    """Stages up to and including the first ``*Encoder`` and the stages after it: the calibration rotation goes
    between them (cli.py:237-250)."""
    if not isinstance(t, MultiTransformer):
        raise ValueError("Automatch requires MultiTransformer")
    names = [type(s).__name__ for s in t.transformers]
    cut = next((i for i, n in enumerate(names) if n.endswith("Encoder")), None)
    if cut is None:
        raise ValueError("Automatch requires a chain with an Encoder stage")
    return MultiTransformer(t.transformers[: cut + 1]), MultiTransformer(t.transformers[cut + 1:])


def _option_number(automatch: str, prefix: str, pattern: str, default: float) -> float:
    """``fm0.5`` -> 0.5, ``gui3`` -> 3, the bare keyword -> ``default`` (cli.py:258-262, 268-274)."""
    m = re.match(prefix + pattern, automatch)
    return float(m.group(1)) if m and m.group(1) else default


def calibrated_pair(transformer: Any, automatch: str, left: Any, right: Any, radius: Any, match_image_path: Optional[Path] = None,
                    center: Any = None) -> tuple[Any, Any]:
    """``--automatch``: estimate the rotation between the eyes from matched points and give each eye half of it
    (cli.py:234-319): (left chain, right chain).  The points come from the option itself (``"xl,yl;xr,yr;..."``: even entries the
    left eye, odd entries the right; plain least-squares fit ``rotation_match``), from clicks (``gui[n]``: n pairs, default 2) or from
    AKAZE feature matching (``fm[scale]``: outlier-ridden, hence ``rotation_match_robust``; ``match_image_path`` = where
    ``--savematch`` wants 100 of the surviving matches drawn).  ``center``: the centres the remap will use (``--center``): the points go
    back through the same ones (``match_lr``)."""
    head, tail = split_at_first_encoder(transformer)
    matched = None
    if automatch.startswith("devfm"):
        # feature matching on the device (features.py): no OpenCV; outlier-ridden like fm, hence the robust fit too
        from . import features as _feat

        scale = _option_number(automatch, "devfm", r"([\d\.]+)", 1)
        if not 0 < scale <= 1:
            raise typer.BadParameter(f"--automatch {automatch}: the working scale must lie in (0, 1], e.g. devfm0.5")
        # (--device-decode hands over the decoded tensors: the matcher takes them where they lie)
        images = [_io.imread(q) if isinstance(q, (str, Path)) else q for q in (left, right)]
        matched = _feat.match_points_device(images[0], images[1], scale=scale, radius=radius)
        points_l, points_r = matched[0], matched[1]
    elif automatch.startswith("fm") or automatch.startswith("gui"):
        from . import calibration_cv as _cvx

        try:
            img_l, img_r = _io.imread(left), _io.imread(right)
            if automatch.startswith("fm"):
                matched = _cvx.match_points(img_l, img_r, scale=_option_number(automatch, "fm", r"([\d\.]+)", 1))
                points_l, points_r = matched[0], matched[1]
            else:
                n_pairs = int(_option_number(automatch, "gui", r"(\d+)", 2))
                clicks = _cvx.pick_points_gui([img_l, img_r] * n_pairs)
                LOG.info("Automatched position: " + ";".join(",".join(map(str, p)) for p in clicks))
                points_l, points_r = clicks[::2], clicks[1::2]
        except _cvx.OptionalDependencyMissing as e:
            raise typer.BadParameter(f'--automatch {automatch}: {e}; or pass the matched points explicitly, e.g. '
                                     '--automatch "xl,yl;xr,yr;xl,yl;xr,yr"') from e
    else:
        flat = [(int(c.split(",")[0]), int(c.split(",")[1])) for c in automatch.split(";")]
        points_l, points_r = flat[::2], flat[1::2]  # even entries: left eye, odd entries: right eye
    vl, vr = match_lr(tail, points_l, points_r, in_paths=[left, right], radius=radius, **({} if center is None else {"center": center}))
    if matched is not None:
        q, discarded = rotation_match_robust(vl, vr)
        if match_image_path is not None and automatch.startswith("fm"):
            from . import calibration_cv as _cvx

            _, _, kp_l, kp_r, matches, small_l, small_r = matched
            _io.imwrite(match_image_path, _cvx.draw_match_image(small_l, kp_l, small_r, kp_r, matches, discarded))
    else:
        q = rotation_match(vl, vr)
    LOG.info(f"Automatched quaternion: {q}")
    q_left, q_right = calibration_rotators(q)
    return head * _T.Euclidean3DRotator(q_left) * tail, head * _T.Euclidean3DRotator(q_right) * tail


@app.callback()
def _main(verbose: bool = typer.Option(False, "--verbose", "-v")) -> None:
    handlers = None
    try:
        from rich.logging import RichHandler

        handlers = [RichHandler(rich_tracebacks=True)]
    except Exception:  # noqa: BLE001
        pass
    logging.basicConfig(level=logging.DEBUG if verbose else logging.INFO, format="%(message)s", datefmt="[%X]", handlers=handlers)


@app.command()
def lr(
    left_path: Annotated[Path, typer.Argument(help="Left image path (or a directory to search for the time-matched image)")],
    right_path: Annotated[Path, typer.Argument(help="Right image path (or a directory)")],
    transformer: Annotated[str, typer.Option(help="Transformer Python code (to be `eval()`ed)")] = "",
    out_path: Annotated[Path, typer.Option(help="Output image path or directory, defaults to <left>-<right>.png next to the left image")] = Path(""),
    size: Annotated[str, typer.Option(help="Output image size per eye")] = "4096x4096",
    interpolation: Annotated[str, typer.Option(help="Interpolation method (cv2 name)")] = "inter_lanczos4",
    border_mode: Annotated[str, typer.Option(help="Border mode (cv2 name)")] = "border_constant",
    border_value: int = 0,
    radius: Annotated[str, typer.Option(help="Radius of the fisheye image: a number, 'auto', 'max' or 'fit' (the fitted image circle's)")] = "auto",
    center: Annotated[str, typer.Option(help="Centre of the image circles in source pixels: 'auto' (fitted per eye), 'X,Y' or "
                                             "'LX,LY;RX,RY' (each in its own eye's coordinates); default: the frame's centre")] = "",
    merge: Annotated[bool, typer.Option("-m", "--merge", "--anaglyph", help="Export as an anaglyph")] = False,
    autosearch_timestamp_calib_r_earlier_l: Annotated[float, typer.Option(
        "--autosearch-timestamp-calib-r-earlier-l", "-ac",
        help="Autosearch timestamp calibration (right timestamp -= this) (in seconds)")] = 0.0,
    swap: Annotated[bool, typer.Option(help="Swap left and right images as well as transformer, etc.")] = False,
    name_unique: Annotated[bool, typer.Option(help="Make output name unique")] = False,
    automatch: Annotated[str, typer.Option(help='Calibrate rotation. e.g. "0,0;0,0;1,1;1,1", "gui[n]" (click n point pairs), '
                                                 '"fm[scale]" (AKAZE feature matching) -- these two need OpenCV -- or "devfm[scale]" '
                                                 '(feature matching on the GPU, no OpenCV; not AKAZE)')] = "",
    savematch: Annotated[bool, typer.Option(help="Save the match image <out>.match<ext> (only with automatch=fm)")] = False,
    device_png: Annotated[bool, typer.Option("--device-png", help="Deflate .png results on the GPU (larger files, no host codec "
                                                                   "time); other formats and --merge are written by the host")] = False,
    device_jpeg: Annotated[bool, typer.Option("--device-jpeg", help="Encode .jpg / .jpeg results on the GPU (baseline JPEG, quality 95, "
                                                                     "4:2:0); other formats and --merge are written by the host")] = False,
    device_jpeg_batch: Annotated[bool, typer.Option("--device-jpeg-batch", help="As --device-jpeg, with all the results encoded in one "
                                                                                 "batch that shares its kernel launches")] = False,
    device_decode: Annotated[bool, typer.Option("--device-decode", help="Decode .jpg / .jpeg inputs on the GPU (baseline JPEG; other "
                                                                         "files are read by the host)")] = False,
    device_decode_batch: Annotated[bool, typer.Option("--device-decode-batch", help="As --device-decode, with all the files decoded in one "
                                                                                     "batch that shares its kernel launches")] = False,
    device_jpeg_optimize: Annotated[bool, typer.Option("--device-jpeg-optimize", help="With --device-jpeg or --device-jpeg-batch: Huffman "
                                                                                       "tables built for each image on the GPU (smaller "
                                                                                       "files, the same pixels)")] = False,
    device_decode_progressive: Annotated[bool, typer.Option("--device-decode-progressive", help="With --device-decode or --device-decode-batch: "
                                                                                                 "progressive JPEG inputs are decoded on "
                                                                                                 "the GPU too")] = False,
    device_vr180: Annotated[bool, typer.Option("--device-vr180", help="Write a .jpg / .jpeg result as a Google VR180 photo: both eyes "
                                                                       "encoded on the GPU, the right eye embedded in the left eye's "
                                                                       "XMP (not with --merge)")] = False,
    match_colors: Annotated[str, typer.Option("--match-colors", help="Match the colours of one eye to the other's on the GPU after the "
                                                                      "remap: 'gain' (one factor per channel) or 'histogram' (the "
                                                                      "distributions); 8-bit images; default: off")] = "",
    match_reference: Annotated[str, typer.Option("--match-reference", help="With --match-colors: the eye of the result that stays as it "
                                                                            "is, 'left' or 'right' (after --swap)")] = "left",
    chromatic: Annotated[str, typer.Option("--chromatic", help="Correct lateral chromatic aberration inside the remap: "
                                                                "'r:c0,c1,...;b:c0,c1,...' -- per channel a polynomial in the normalised "
                                                                "source radius (1.0 = the rim), lowest order first; 'LEFT|RIGHT' for one "
                                                                "per eye (swapped by --swap); 8-bit BGR images; default: off")] = "",
    vignette: Annotated[str, typer.Option("--vignette", help="Correct lens vignetting on the GPU in front of the remap: 'k1,k2,k3' of "
                                                              "V = 1 + k1 r^2 + k2 r^4 + k3 r^6 (r = 1.0 at the rim), "
                                                              "'b:..;g:..;r:..' per channel, 'LEFT|RIGHT' for one per eye (swapped by "
                                                              "--swap); 8- and 16-bit images; the `vignette` command fits them; "
                                                              "default: off")] = "",
    vignette_gamma: Annotated[float, typer.Option("--vignette-gamma", help="With --vignette: the power-law encoding of the pixels, 1.0 for "
                                                                           "linear light, 2.2 for the usual 8-bit files")] = 1.0,
) -> None:
    """Remap a pair of fisheye images to a pair of SBS equirectangular images."""
    from .remapper import apply_lr

    chromatic_ = parse_chromatic(chromatic, swap=swap)
    vignette_ = parse_vignette(vignette, vignette_gamma, swap=swap)

    if match_colors not in ("", "gain", "histogram"):
        raise typer.BadParameter(f"--match-colors {match_colors}: expected 'gain' or 'histogram'")
    if match_reference not in ("left", "right"):
        raise typer.BadParameter(f"--match-reference {match_reference}: expected 'left' or 'right'")

    r_earlier_l = autosearch_timestamp_calib_r_earlier_l
    if swap:
        left_path, right_path, r_earlier_l = right_path, left_path, -r_earlier_l
    left_path, right_path = resolve_pair(left_path, right_path, r_earlier_l)
    LOG.info("L: %s@%s, R: %s@%s", left_path, datetime.fromtimestamp(left_path.stat().st_mtime, timezone.utc),
             right_path, datetime.fromtimestamp(right_path.stat().st_mtime, timezone.utc))
    interp = _flag(interpolation, _INTERPOLATIONS, "inter_", "interpolation")
    border = _flag(border_mode, _BORDERS, "border_", "border mode")
    radius_ = parse_radius(radius)
    center_ = parse_center(center, swap=swap)
    chain: Any = parse_transformer(transformer)
    # (the reference hashes the option AFTER --swap negated it, cli.py:174-176, 347: str(-0.0) == "-0.0" even for the default)
    tag = unique_suffix(transformer, size, interpolation, border_mode, border_value, radius, merge,
                        r_earlier_l, swap) if name_unique else ""
    out = output_path(out_path, left_path, right_path, tag)
    if savematch and not automatch.startswith("fm"):
        # (the reference ignores the flag silently, cli.py:365: scripts that always pass it keep working)
        LOG.warning("--savematch ignored: it draws the feature matches of --automatch fm, and there are none without it")
    left_in: Any = left_path
    right_in: Any = right_path
    if (device_decode or device_decode_batch) and automatch.startswith("devfm") and left_path != right_path:
        # decoded once, here: the matcher and apply_lr both take the tensors (apply_lr passes what is no path through)
        from . import jpeg_decode_device

        left_in, right_in = jpeg_decode_device.read_inputs([left_path, right_path], **({"batch": True} if device_decode_batch else {}),
                                                                **({"progressive": True} if device_decode_progressive else {}))
    if automatch != "":
        match_image = out.with_suffix(f".match{out.suffix}") if savematch else None  # cli.py:362-365
        if center_ is not None and isinstance(left_in, Path) and left_in == right_in:
            # one file holding both eyes: the centres are in each half's own coordinates, so the calibration sees the halves too
            both = _io.imread(left_in)
            left_in, right_in = both[:, : both.shape[1] // 2], both[:, both.shape[1] // 2:]
        chain = calibrated_pair(chain, automatch, left_in, right_in, radius_, match_image, **({} if center_ is None else {"center": center_}))
        LOG.info(f"Automatched transformer: {chain}")
    apply_lr(chain, left_path=left_in, right_path=right_in, out_path=out, radius=radius_, size_output=parse_size(size),
             interpolation=interp, boarder_mode=border, boarder_value=border_value, merge=merge,
             **({} if center_ is None else {"center": center_}),
             **({"device_png": True} if device_png else {}),
             **({"device_jpeg": "vr180"} if device_vr180 else {"device_jpeg": "batch"} if device_jpeg_batch else {"device_jpeg": True} if device_jpeg else {}),
             **({"device_decode": "batch"} if device_decode_batch else {"device_decode": True} if device_decode else {}),
             **({"device_jpeg_optimize": True} if device_jpeg_optimize else {}),
             **({"device_decode_progressive": True} if device_decode_progressive else {}),
             **({"match_colors": match_colors, "match_reference": match_reference} if match_colors else {}),
             **({} if chromatic_ is None else {"chromatic": chromatic_}),
             **({} if vignette_ is None else {"vignette": vignette_}))


@app.command()
def s(
    in_paths: Annotated[List[Path], typer.Argument(help="Image paths")],
    transformer: Annotated[str, typer.Option(help="Transformer Python code (to be `eval()`ed)")] = "",
    out_path: Annotated[Path, typer.Option(help="Output image path or directory, defaults to <in>.out.png")] = Path(""),
    size: Annotated[str, typer.Option(help="Output image size")] = "4096x4096",
    interpolation: Annotated[str, typer.Option(help="Interpolation method (cv2 name)")] = "inter_lanczos4",
    boarder_mode: Annotated[str, typer.Option(help="Border mode (cv2 name)")] = "border_constant",
    boarder_value: int = 0,
    radius: Annotated[str, typer.Option(help="Radius of the fisheye image: a number, 'auto', 'max' or 'fit' (the fitted image circle's)")] = "auto",
    center: Annotated[str, typer.Option(help="Centre of the image circle in source pixels: 'auto' (fitted per image) or 'X,Y'; "
                                             "default: the frame's centre")] = "",
    device_png: Annotated[bool, typer.Option("--device-png", help="Deflate .png results on the GPU (larger files, no host codec "
                                                                   "time); other formats and --merge are written by the host")] = False,
    device_jpeg: Annotated[bool, typer.Option("--device-jpeg", help="Encode .jpg / .jpeg results on the GPU (baseline JPEG, quality 95, "
                                                                     "4:2:0); other formats are written by the host")] = False,
    device_jpeg_batch: Annotated[bool, typer.Option("--device-jpeg-batch", help="As --device-jpeg, with all the results encoded in one "
                                                                                 "batch that shares its kernel launches")] = False,
    device_decode: Annotated[bool, typer.Option("--device-decode", help="Decode .jpg / .jpeg inputs on the GPU (baseline JPEG; other "
                                                                         "files are read by the host)")] = False,
    device_decode_batch: Annotated[bool, typer.Option("--device-decode-batch", help="As --device-decode, with all the files decoded in one "
                                                                                     "batch that shares its kernel launches")] = False,
    device_jpeg_optimize: Annotated[bool, typer.Option("--device-jpeg-optimize", help="With --device-jpeg or --device-jpeg-batch: Huffman "
                                                                                       "tables built for each image on the GPU (smaller "
                                                                                       "files, the same pixels)")] = False,
    device_decode_progressive: Annotated[bool, typer.Option("--device-decode-progressive", help="With --device-decode or --device-decode-batch: "
                                                                                                 "progressive JPEG inputs are decoded on "
                                                                                                 "the GPU too")] = False,
    chromatic: Annotated[str, typer.Option("--chromatic", help="Correct lateral chromatic aberration inside the remap: "
                                                                "'r:c0,c1,...;b:c0,c1,...' -- per channel a polynomial in the normalised "
                                                                "source radius (1.0 = the rim), lowest order first; 8-bit BGR images; "
                                                                "default: off")] = "",
    vignette: Annotated[str, typer.Option("--vignette", help="Correct lens vignetting on the GPU in front of the remap: 'k1,k2,k3' of "
                                                              "V = 1 + k1 r^2 + k2 r^4 + k3 r^6 (r = 1.0 at the rim) or "
                                                              "'b:..;g:..;r:..' per channel; 8- and 16-bit images; default: off")] = "",
    vignette_gamma: Annotated[float, typer.Option("--vignette-gamma", help="With --vignette: the power-law encoding of the pixels, 1.0 for "
                                                                           "linear light, 2.2 for the usual 8-bit files")] = 1.0,
) -> None:
    """Remap fisheye images to equirectangular images (one shared map for all of them)."""
    from .remapper import apply

    chromatic_ = parse_chromatic(chromatic, pair=False)
    vignette_ = parse_vignette(vignette, vignette_gamma, pair=False)

    if out_path == Path(""):
        out_paths = [p.with_suffix(f".out.{DEFAULT_EXTENSION}") for p in in_paths]
    elif out_path.is_dir():
        out_paths = [out_path / p.name for p in in_paths]
    elif len(in_paths) > 1:
        raise ValueError("Output path must be a directory when multiple input paths are provided")
    else:
        out_paths = [out_path]
    apply(parse_transformer(transformer), in_paths=list(in_paths), out_paths=out_paths, radius=parse_radius(radius),
          size_output=parse_size(size), interpolation=_flag(interpolation, _INTERPOLATIONS, "inter_", "interpolation"),
          boarder_mode=_flag(boarder_mode, _BORDERS, "border_", "border mode"), boarder_value=boarder_value,
          **({} if center == "" else {"center": parse_center(center, pair=False)}),
          **({"device_png": True} if device_png else {}), **({"device_jpeg": "batch"} if device_jpeg_batch else {"device_jpeg": True} if device_jpeg else {}),
          **({"device_decode": "batch"} if device_decode_batch else {"device_decode": True} if device_decode else {}),
          **({"device_jpeg_optimize": True} if device_jpeg_optimize else {}),
          **({"device_decode_progressive": True} if device_decode_progressive else {}),
          **({} if chromatic_ is None else {"chromatic": chromatic_}),
          **({} if vignette_ is None else {"vignette": vignette_}))


@app.command(name="vignette")
def vignette_fit(
    flat_path: Annotated[Path, typer.Argument(help="A flat-field frame of the lens: a white wall, an overcast sky, a diffuser over the lens")],
    center: Annotated[str, typer.Option(help="Centre of the image circle in source pixels: 'auto' (fitted) or 'X,Y'; default: the frame's "
                                             "centre")] = "",
    radius: Annotated[str, typer.Option(help="Radius of the image circle: a number or 'fit' (the fitted image circle's)")] = "fit",
    rings: Annotated[int, typer.Option(help="Rings of equal area the statistics are gathered in, 16..1024")] = 256,
    gamma: Annotated[float, typer.Option(help="The power-law encoding of the frame's pixels: 1.0 for linear light, 2.2 for the usual 8-bit "
                                              "files; pass the same value as --vignette-gamma")] = 1.0,
) -> None:
    """Fit the vignetting of a lens from a flat-field frame on the GPU and print the coefficients in the form --vignette reads."""
    from . import vignette

    radius_: Any = "fit" if radius == "fit" else float(radius)
    center_: Any = None if center == "" else parse_center(center, pair=False)
    try:
        v = vignette.fit_vignette(_io.imread(flat_path), center=center_, radius=radius_, rings=rings, gamma=gamma)
    except ValueError as e:
        raise typer.BadParameter(str(e)) from e
    typer.echo(v.spec())


@app.command()
def swap(
    in_paths: Annotated[List[Path], typer.Argument(help="Image paths")],
    overwrite: Annotated[bool, typer.Option(help="Overwrite the original images")] = True,
    lossless: Annotated[bool, typer.Option("--lossless", help="Exchange the halves of .jpg / .jpeg files in the DCT domain on the GPU: "
                                                               "no pixel changes, no JPEG generation is lost (the halves must be whole "
                                                               "MCUs wide; other files are decoded and encoded again as without it)")] = False,
) -> None:
    """Swap the left and right halves of side-by-side images."""
    for p in in_paths:
        if lossless and p.suffix.lower() in (".jpg", ".jpeg"):
            from . import jpeg_transcode_device as _xc

            from .jpeg_decode_device import CorruptJPEG

            try:
                swapped = _xc.swap_sbs_jpeg(p.read_bytes())
            except CorruptJPEG as e:  # a damaged file has no other route: said here, where the message names the byte
                raise typer.BadParameter(f"{p}: {e}") from e
            except (NotImplementedError, ValueError) as e:  # outside the transcoder's scope, or halves off the MCU grid: said, then as ever
                LOG.warning(f"--lossless: {p} is decoded and encoded again: {e}")
            else:
                (p if overwrite else p.with_suffix(f".swap{p.suffix}")).write_bytes(swapped)
                continue
        image = _io.imread(p)
        if image is None:
            raise ValueError(f"cannot read {p}")
        half = image.shape[1] // 2
        _io.imwrite(p if overwrite else p.with_suffix(f".swap{p.suffix}"), np.hstack([image[:, half:], image[:, :half]]))


@app.command()
def xmp(
    in_paths: Annotated[List[Path], typer.Argument(help="Side-by-side image paths")],
    wslpath: Annotated[bool, typer.Option("-wsl", "--wslpath", help="Convert Windows paths to WSL paths (runs `wslpath`)")] = False,
    device: Annotated[bool, typer.Option("--device", help="Split .jpg / .jpeg files in the DCT domain on the GPU and write the XMP "
                                                           "here: no pixel changes, no libxmp (the halves must be whole MCUs wide; "
                                                           "other files take the route without it)")] = False,
) -> None:
    """Write the left half as <name>.xmp<ext> with the right half embedded as Google VR180 photo metadata
    (GPano / GImage XMP, cli.py:439-540).  Needs python-xmp-toolkit (libxmp / exempi) unless --device takes the file."""
    import subprocess as sp

    from . import calibration_cv as _cvx

    for in_path in in_paths:
        if wslpath:  # cli.py:477-482
            in_path = Path(sp.run(["wslpath", "-u", "-a", str(in_path)], capture_output=True).stdout.decode().strip())  # noqa: S603, S607
        if device and in_path.suffix.lower() in (".jpg", ".jpeg"):
            from . import jpeg_transcode_device as _xc, vr180_photo as _vp

            from .jpeg_decode_device import CorruptJPEG

            try:
                data = in_path.read_bytes()  # (read once: the size and the split take the bytes)
                height, width, _, _ = _xc.probe_mcu(data)
                left, right = _xc.split_sbs_jpeg(data)
            except CorruptJPEG as e:  # a damaged file has no other route: said here, where the message names the byte
                raise typer.BadParameter(f"{in_path}: {e}") from e
            except (NotImplementedError, ValueError) as e:  # outside the transcoder's scope, or halves off the MCU grid: said, then as ever
                LOG.warning(f"--device: {in_path} takes the host route: {e}")
            else:
                written = in_path.with_suffix(f".xmp{in_path.suffix}")
                written.write_bytes(_vp.assemble_vr180_photo(left, right, width, height))
                LOG.info(f"Saved {written}")
                continue
        try:
            written = _cvx.write_vr180_xmp(in_path)
        except _cvx.OptionalDependencyMissing as e:
            raise typer.BadParameter(str(e)) from e
        LOG.info(f"Saved {written}")


@app.command()
def join(
    in_paths: Annotated[List[Path], typer.Argument(help="LEFT RIGHT: the two eyes' .jpg / .jpeg files; or one Google VR180 photo")],
    left_transform: Annotated[Optional[str], typer.Option("--left-transform", help="flip_h, flip_v, rot180, transpose, rot90 (clockwise), "
                                                                                    "rot270 or transverse: applied to the left eye")] = None,
    right_transform: Annotated[Optional[str], typer.Option("--right-transform", help="As --left-transform, for the right eye")] = None,
    trim: Annotated[bool, typer.Option("--trim", help="Cut a partial last MCU column or row off where a mirror or the join needs whole "
                                                      "MCUs, instead of refusing")] = False,
    optimize: Annotated[bool, typer.Option("--optimize", help="Huffman tables built for the output on the GPU")] = False,
    vr180: Annotated[bool, typer.Option("--vr180", help="Write the transformed eyes as a Google VR180 photo instead of side by side")] = False,
    out_path: Annotated[Optional[Path], typer.Option("--out-path", help="Default: LEFT's name with .join (or .sbs for a VR180 photo) in "
                                                                        "front of its suffix")] = None,
) -> None:
    """Join two per-eye JPEG files into one side-by-side file in the DCT domain on the GPU, each eye flipped or rotated on the way: no
    pixel is decoded, no JPEG generation is lost.  With one argument, a Google VR180 photo, write its side-by-side file."""
    from . import jpeg_compose_device as _xf, vr180_photo as _vp

    from .jpeg_decode_device import CorruptJPEG

    if len(in_paths) not in (1, 2):
        raise typer.BadParameter("join takes LEFT RIGHT, or one VR180 photo")
    try:
        if len(in_paths) == 1:
            left, right, _ = _vp.read_vr180_photo(in_paths[0].read_bytes())
        else:
            left, right = in_paths[0].read_bytes(), in_paths[1].read_bytes()
        kw = dict(trim=trim, optimize=optimize)
        if vr180:
            eyes = [_xf.transform_jpeg(eye, t or "none", **kw) for eye, t in ((left, left_transform), (right, right_transform))]
            (lh, lw, _, _), (rh, rw, _, _) = (_xf.probe_mcu(eye) for eye in eyes)
            if lh != rh:
                raise ValueError(f"the eyes end up {lh} and {rh} pixels high: a VR180 photo needs one height")
            made = _vp.assemble_vr180_photo(eyes[0], eyes[1], lw + rw, lh)
        else:
            made = _xf.join_sbs_jpeg(left, right, left_transform=left_transform, right_transform=right_transform, **kw)
    except (CorruptJPEG, NotImplementedError, ValueError) as e:  # nothing falls back: a join through pixels would lose a generation
        raise typer.BadParameter(f"{in_paths[0]}: {e}") from e
    p = in_paths[0]
    written = out_path or p.with_suffix(f"{'.sbs' if len(in_paths) == 1 and not vr180 else '.join'}{p.suffix}")
    written.write_bytes(made)
    LOG.info(f"Saved {written}")


def main(argv: Optional[Sequence[str]] = None) -> None:
    app(args=None if argv is None else list(argv), prog_name="vr180-convert")
