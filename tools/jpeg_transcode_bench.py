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

With ``--transform OP`` (repeatable) and ``--join`` the jobs are the composer's instead (jpeg_compose_device.transform_jpeg,
join_sbs_jpeg): the whole file flipped or rotated, and the join of its two halves (split beforehand, outside the clocks), against
(a) ``decode_jpeg_tensor``, a torch flip / transpose, ``encode_jpeg_tensor`` and (b) Pillow's ``transpose`` / ``hstack``; the PSNR is
taken after the pixels are turned back.  A job ``whole`` -- ``transcode_jpeg`` of the same file, whose gather is ``k_jxc_gather`` over the
same blocks -- runs beside them, so that one profiler session holds both gathers.

    python tools/jpeg_transcode_bench.py --out profiles/jpeg_transcode/bench.jsonl
    python tools/jpeg_transcode_bench.py --transform rot180 --transform rot90 --join --out profiles/jpeg_compose/bench.jsonl
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


def compose_jobs(V, data: bytes, w: int, sampling: int, sub: str, transforms: list, join: bool) -> dict:
    """job: (the composer's call, the device codecs' path, Pillow's path, the pixels of the made files turned back to the source's)"""
    from PIL import Image

    from vr180_convert_amd.jpeg_compose_device import TRANSFORMS

    def turned(x, code, flip, swap):  # transpose first, then mirror x, then mirror y
        if code & 4:
            x = swap(x)
        if code & 1:
            x = flip(x, 1)
        if code & 2:
            x = flip(x, 0)
        return x

    inverse = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 5, 7: 7}
    jobs = {"whole": (lambda **kw: [V.transcode_jpeg(data, **kw)],
                      lambda: [V.encode_jpeg_tensor(V.decode_jpeg_tensor(data), quality=95, subsampling=sub)],
                      lambda: [_save(_pixels(data), sampling)], lambda px: px[0])}
    for op in transforms:
        code = TRANSFORMS[op]
        jobs[op] = (lambda op=op, **kw: [V.transform_jpeg(data, op, **kw)],
                    lambda code=code: [V.encode_jpeg_tensor(turned(V.decode_jpeg_tensor(data), code, lambda x, d: x.flip(d), lambda x: x.transpose(0, 1)).contiguous(),
                                                            quality=95, subsampling=sub)],
                    lambda code=code: [_save(np.ascontiguousarray(turned(_pixels(data), code, lambda x, d: np.flip(x, d), lambda x: np.swapaxes(x, 0, 1))), sampling)],
                    lambda px, code=code: turned(px[0], inverse[code], lambda x, d: np.flip(x, d), lambda x: np.swapaxes(x, 0, 1)))
    if join:
        left, right = V.split_sbs_jpeg(data)
        jobs["join"] = (lambda **kw: [V.join_sbs_jpeg(left, right, **kw)],
                        lambda: [V.encode_jpeg_tensor(torch.cat([V.decode_jpeg_tensor(left), V.decode_jpeg_tensor(right)], dim=1), quality=95, subsampling=sub)],
                        lambda: [_save(np.ascontiguousarray(np.hstack([_pixels(left), _pixels(right)])), sampling)], lambda px: px[0])
    return jobs


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="*", help="side-by-side JPEG files (default: the docs image and an 8192 x 4096 sphere scene)")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--device-only", action="store_true", help="the transcoder and path (a) only, no PSNR (profiler runs)")
    ap.add_argument("--transform", action="append", default=[], metavar="OP", help="the composer's jobs instead: the whole file under OP (repeatable)")
    ap.add_argument("--join", action="store_true", help="the composer's jobs instead: the join of the file's two halves")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_transcode_bench needs the MI355X")
    import vr180_convert_amd as V
    from vr180_convert_amd import jpeg_transcode_device as T
    from vr180_convert_amd.jpeg_compose_device import last_compose_report

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
        if a.transform or a.join:
            jobs = compose_jobs(V, data, w, sampling, sub, a.transform, a.join)
        for job, (xc, codecs, pillow, back) in jobs.items():
            made = xc()  # warm-up: code objects, the page-locked buffer, the memory pool
            rounds = T.last_transcode_report()["rounds"] if job in ("split", "swap", "whole") else [r["rounds"] for r in last_compose_report()["sources"]]
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
