"""Side-by-side JPEG file -> its two halves / its halves exchanged: the lossless transcoder (jpeg_transcode_device.split_sbs_jpeg,
swap_sbs_jpeg) against the two paths it replaces, for the given files or, without any, for the docs side-by-side image
(tests/golden/ref_docs/test.lr.PolynomialScaler.jpg, 4096 x 2048) and an 8192 x 4096 4:2:0 quality-95 file written by Pillow from the
sphere scene:

  (a) the same job through the device codecs: ``decode_jpeg_tensor``, then ``encode_jpeg_tensors`` of the two halves (split) or
      ``encode_jpeg_tensor`` of the halves exchanged (swap), quality 95;
  (b) Pillow on the host: decode, slice, save at quality 95 with the file's sampling -- the two halves of a split in two threads.

For every file and job: ``--runs`` calls after a warm-up, each between two device events and inside a host clock; the rounds of the
decode; path (b) three times.  Generation loss: the PSNR of Pillow's pixels of each path's output against Pillow's pixels of the
source (infinite where every sample is the same).  The size of the transcoder's files with the Annex K tables and with
``optimize=True``.  One JSON line per (file, job); ``--out`` appends them to a file.

    python tools/jpeg_transcode_bench.py --out profiles/jpeg_transcode/bench.jsonl
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/jpeg_transcode_bench.py --runs 2 --device-only     (per-kernel times)
"""
from __future__ import annotations

import argparse
import io
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def default_files() -> dict:
    import sphere_scene as S
    from PIL import Image

    big = np.kron(S.render(2048), np.ones((2, 4, 1), np.uint8))  # 4096 x 8192: the scene at twice the height and four times the width
    big = (big.astype(np.int16) + np.random.default_rng(0).integers(-6, 7, big.shape, dtype=np.int16)).clip(0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(big[..., ::-1])).save(b, "JPEG", quality=95, subsampling=2)
    return {"docs_sbs_4096x2048": (ROOT / "tests" / "golden" / "ref_docs" / "test.lr.PolynomialScaler.jpg").read_bytes(),
            "sphere_8192x4096_q95_420": b.getvalue()}


def _timed(fn) -> tuple:
    """(result, milliseconds between two device events, milliseconds on the host clock until the second event has passed)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0)


def _spread(v: list) -> list:
    v = sorted(v)
    return [round(v[0], 3), round(v[len(v) // 2], 3), round(v[-1], 3)]


def _pixels(data: bytes) -> np.ndarray:
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _psnr(a: np.ndarray, b: np.ndarray) -> float | None:
    """None stands for infinite: every sample is the same"""
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return None if mse == 0 else round(10 * np.log10(255.0 ** 2 / mse), 2)


def _save(arr: np.ndarray, sampling: int) -> bytes:
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(arr).save(b, "JPEG", quality=95, subsampling=sampling)
    return b.getvalue()


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="*", help="side-by-side JPEG files (default: the docs image and an 8192 x 4096 sphere scene)")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--device-only", action="store_true", help="the transcoder and path (a) only, no PSNR (profiler runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_transcode_bench needs the MI355X")
    import vr180_convert_amd as V
    from vr180_convert_amd import jpeg_transcode_device as T

    files = {Path(f).name: Path(f).read_bytes() for f in a.files} if a.files else default_files()
    for name, data in files.items():
        h, w, mw, mh = T.probe_mcu(data)
        sampling = {(8, 8): 0, (16, 8): 1, (16, 16): 2}[(mw, mh)]
        sub = "420" if sampling == 2 else "444"
        source = None if a.device_only else _pixels(data)

        def codecs_split():
            t = V.decode_jpeg_tensor(data)
            return V.encode_jpeg_tensors([t[:, :w // 2], t[:, w // 2:]], quality=95, subsampling=sub)

        def codecs_swap():
            t = V.decode_jpeg_tensor(data)
            return [V.encode_jpeg_tensor(torch.cat([t[:, w // 2:], t[:, :w // 2]], dim=1), quality=95, subsampling=sub)]

        def pillow_split():
            arr = _pixels(data)
            with ThreadPoolExecutor(2) as pool:
                return list(pool.map(lambda x: _save(np.ascontiguousarray(x), sampling), (arr[:, :w // 2], arr[:, w // 2:])))

        def pillow_swap():
            arr = _pixels(data)
            return [_save(np.ascontiguousarray(np.hstack([arr[:, w // 2:], arr[:, :w // 2]])), sampling)]

        jobs = {"split": (lambda **kw: list(V.split_sbs_jpeg(data, **kw)), codecs_split, pillow_split,
                          lambda px: np.hstack(px)),
                "swap": (lambda **kw: [V.swap_sbs_jpeg(data, **kw)], codecs_swap, pillow_swap,
                         lambda px: np.hstack([px[0][:, w // 2:], px[0][:, :w // 2]]))}
        for job, (xc, codecs, pillow, back) in jobs.items():
            made = xc()  # warm-up: code objects, the page-locked buffer, the memory pool
            rounds = T.last_transcode_report()["rounds"]
            via = codecs()
            dec_rounds = V.last_decode_report()["rounds"]
            torch.cuda.synchronize()
            t_xc, t_a = [], []
            for _ in range(a.runs):  # (alternating, so that a drift of the clocks meets both alike)
                _, ev, host = _timed(xc)
                t_xc.append((ev, host))
                _, ev, host = _timed(codecs)
                t_a.append((ev, host))
            line = {"file": name, "bytes": len(data), "shape": [h, w], "mcu": [mw, mh], "job": job, "runs": a.runs,
                    "transcode_rounds": rounds, "codecs_decode_rounds": dec_rounds,
                    "transcode_events_ms_min_median_max": _spread([t[0] for t in t_xc]),
                    "transcode_host_ms_min_median_max": _spread([t[1] for t in t_xc]),
                    "codecs_events_ms_min_median_max": _spread([t[0] for t in t_a]),
                    "codecs_host_ms_min_median_max": _spread([t[1] for t in t_a]),
                    "transcode_bytes": [len(f) for f in made], "codecs_bytes": [len(f) for f in via]}
            line["codecs_over_transcode_median_host"] = round(line["codecs_host_ms_min_median_max"][1] / line["transcode_host_ms_min_median_max"][1], 3)
            if not a.device_only:
                t_b = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    host_made = pillow()
                    t_b.append(1e3 * (time.perf_counter() - t0))
                line["pillow_ms_min_median_max"] = _spread(t_b)
                line["pillow_bytes"] = [len(f) for f in host_made]
                line["psnr_db_transcode"] = _psnr(back([_pixels(f) for f in made]), source)
                line["psnr_db_codecs"] = _psnr(back([_pixels(f) for f in via]), source)
                line["psnr_db_pillow"] = _psnr(back([_pixels(f) for f in host_made]), source)
                line["transcode_optimize_bytes"] = [len(f) for f in xc(optimize=True)]
            text = json.dumps(line)
            print(text, flush=True)
            if a.out:
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(text + "\n")


if __name__ == "__main__":
    main()
