"""Device tensor -> JPEG bytes on the host: the device encoder (jpeg_device.encode_jpeg_tensor) on a C2-sized side-by-side result
(8192 x 4096 x 3, the remap of a sphere-scene pair) at quality 95, 4:2:0 and 4:4:4, against the path it replaces (``t.cpu().numpy()`` +
Pillow at the same quality and subsampling).

``--runs`` calls after a warm-up, over rotated copies of the result (as bench.py rotates its buffers), each between two device events
and inside a host clock; the call ends in a device synchronisation, so the two agree but for the copy of the scan.  One JSON line per
subsampling; ``--out`` appends them to a file.

``--batch N [N ...]``: after those lines, one ``encode_jpeg_tensors`` call over N single-eye results of ``--batch-size`` squared
(default 2048) against N ``encode_jpeg_tensor`` calls in the same process; ``--batch-frames N [N ...]``: the same over N copies of the
side-by-side frame.  Both ways are warmed up, then alternate run by run (``--batch-runs``, at least 7); each run lies between two
device events and inside a host clock, and every line carries min / median / max of both, the chunks the batch took and
``equal_to_single``.  ``--no-single`` leaves the single-frame lines out.

``--optimize``: every line twice, with the Annex K tables and with optimised tables (``optimize=True``; the line says which); the two
arms of a single-image line alternate run by run in the same process.  ``--eye``: single-call lines for one single-eye result of
``--batch-size`` squared as well.

    python tools/jpeg_device_bench.py --out profiles/jpeg_device/bench.jsonl
    python tools/jpeg_device_bench.py --runs 10 --device-only --batch 2 16 64 --batch-frames 2 4 --out profiles/jpeg_encode_batch/bench.jsonl
    python tools/jpeg_device_bench.py --runs 10 --device-only --optimize --eye --batch 16 --out profiles/jpeg_encode_opt/bench.jsonl
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/jpeg_device_bench.py --runs 2 --device-only     (per-kernel times)
"""
from __future__ import annotations

import argparse
import io
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def result(size: int, dev: torch.device) -> torch.Tensor:
    import sphere_scene as S
    import vr180_convert_amd as V
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder

    src = min(size, 2048)
    left, right = S.render(src), S.render(src, S.rotation([0.3, 1, 0.2], 4))
    sbs = V.apply_lr_tensors(EquirectangularEncoder() * FisheyeDecoder("equidistant"), torch.from_numpy(left).to(dev),
                             torch.from_numpy(right).to(dev), size_output=(size, size), interpolation=1, radius="max")
    torch.cuda.synchronize()
    return sbs


def _mmm(v: list[float]) -> list[float]:
    v = sorted(v)
    return [round(v[0], 3), round(v[len(v) // 2], 3), round(v[-1], 3)]


def batch_lines(images: list[torch.Tensor], what: str, a, optimize: bool = False) -> dict:
    """one encode_jpeg_tensors call against len(images) encode_jpeg_tensor calls, alternating"""
    import vr180_convert_amd as V

    kw = {"optimize": True} if optimize else {}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return out, e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0)

    def loop():
        return [V.encode_jpeg_tensor(t, quality=a.quality, subsampling=a.batch_subsampling, **kw) for t in images]

    def batch():
        return V.encode_jpeg_tensors(images, quality=a.quality, subsampling=a.batch_subsampling, **kw)

    single, _, _ = timed(loop)   # warm-up of both: code objects, the page-locked buffer, the memory pool
    together, _, _ = timed(batch)
    chunks = V.last_encode_batch_report()["chunks"]
    equal = single == together
    nbytes = sum(len(f) for f in together)
    del single, together
    torch.cuda.synchronize()
    ev = {"loop": [], "batch": []}
    host = {"loop": [], "batch": []}
    for k in range(max(7, a.batch_runs)):
        for name, fn in (("loop", loop), ("batch", batch)) if k % 2 == 0 else (("batch", batch), ("loop", loop)):
            _, e, h = timed(fn)
            ev[name].append(e), host[name].append(h)
    h, w, cn = (int(v) for v in images[0].shape)
    return {"batch_of": what, "n": len(images), "shape": [h, w, cn], "quality": a.quality, "subsampling": a.batch_subsampling,
            "optimize": optimize, "jpeg_bytes": nbytes, "runs": len(ev["loop"]), "chunks": chunks, "equal_to_single": equal,
            "loop_events_ms_min_median_max": _mmm(ev["loop"]), "batch_events_ms_min_median_max": _mmm(ev["batch"]),
            "loop_host_ms_min_median_max": _mmm(host["loop"]), "batch_host_ms_min_median_max": _mmm(host["batch"]),
            "loop_over_batch_median": round(_mmm(ev["loop"])[1] / _mmm(ev["batch"])[1], 3)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=4096, help="output size per eye")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--device-only", action="store_true", help="skip the host path (profiler runs)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, nargs="+", default=[], help="list lengths of single-eye results for the batch comparison")
    ap.add_argument("--batch-frames", type=int, nargs="+", default=[], help="list lengths of side-by-side frames for the batch comparison")
    ap.add_argument("--batch-size", type=int, default=2048, help="size of a single-eye result of --batch")
    ap.add_argument("--batch-runs", type=int, default=7)
    ap.add_argument("--batch-subsampling", default="420")
    ap.add_argument("--no-single", action="store_true", help="skip the single-frame lines")
    ap.add_argument("--optimize", action="store_true", help="every line with the Annex K tables and with optimised tables")
    ap.add_argument("--eye", action="store_true", help="single-call lines for one single-eye result of --batch-size squared too")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_device_bench needs the MI355X")
    from PIL import Image

    import vr180_convert_amd as V

    dev = torch.device("cuda", 0)
    sbs = result(a.size, dev)
    copies = [sbs.clone() for _ in range(3)]
    h, w, cn = (int(v) for v in sbs.shape)
    def emit(line: dict) -> None:
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")

    arms = (False, True) if a.optimize else (False,)
    singles = [] if a.no_single else [(sbs, copies)]
    if a.eye:
        eye1 = result(a.batch_size, dev)[:, :a.batch_size].contiguous()
        singles.append((eye1, [eye1.clone() for _ in range(3)]))
    for image, rotated in singles:
        h, w, cn = (int(v) for v in image.shape)
        for sub in ("420", "444"):
            def device_path(t, optimize):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                data = V.encode_jpeg_tensor(t, quality=a.quality, subsampling=sub, **({"optimize": True} if optimize else {}))
                e1.record()
                e1.synchronize()
                return data, {"events_ms": e0.elapsed_time(e1), "host_ms": 1e3 * (time.perf_counter() - t0)}

            def host_path(t):
                t0 = time.perf_counter()
                host = t.cpu().numpy()
                t1 = time.perf_counter()
                b = io.BytesIO()
                Image.fromarray(np.ascontiguousarray(host[..., ::-1])).save(b, "JPEG", quality=a.quality, subsampling={"420": 2, "444": 0}[sub])
                t2 = time.perf_counter()
                return b.getvalue(), {"copy_ms": 1e3 * (t1 - t0), "encode_ms": 1e3 * (t2 - t1), "total_ms": 1e3 * (t2 - t0)}

            jpg_d = {o: device_path(rotated[0], o)[0] for o in arms}  # warm-up: code objects, the page-locked buffer, the memory pool
            jpg_h = None if a.device_only else host_path(rotated[0])[0]
            torch.cuda.synchronize()
            drun, hrun = {o: [] for o in arms}, []
            for k in range(a.runs):
                for o in arms if k % 2 == 0 else arms[::-1]:  # the arms alternate, run by run
                    drun[o].append(device_path(rotated[k % 3], o)[1])
                if not a.device_only and k < 3:
                    hrun.append(host_path(rotated[k % 3])[1])
            for o in arms:
                dec = np.asarray(Image.open(io.BytesIO(jpg_d[o])))[..., ::-1].astype(np.float64)
                mse = float(np.mean((dec - image.cpu().numpy()) ** 2))
                ev = sorted(r["events_ms"] for r in drun[o])
                line = {"shape": [h, w, cn], "quality": a.quality, "subsampling": sub, "optimize": o, "runs": a.runs, "raw_bytes": h * w * cn,
                        "device_jpeg_bytes": len(jpg_d[o]), "host_jpeg_bytes": None if jpg_h is None else len(jpg_h),
                        "psnr_db": round(10 * np.log10(255.0 ** 2 / max(mse, 1e-12)), 2),
                        "events_ms_min_median_max": [round(ev[0], 3), round(ev[len(ev) // 2], 3), round(ev[-1], 3)],
                        "mpixel_per_s_median": round(h * w / 1e3 / ev[len(ev) // 2], 1), "device": drun[o], "host": hrun}
                emit(line)

    if a.batch:
        eye = result(a.batch_size, dev)[:, :a.batch_size]
        for n in a.batch:  # (distinct images: every one the eye shifted by some rows)
            for o in arms:
                emit(batch_lines([torch.roll(eye, 8 * k, 0).contiguous() for k in range(n)], "eye", a, o))
    for n in a.batch_frames:
        for o in arms:
            emit(batch_lines([sbs] + [torch.roll(sbs, 16 * k, 0) for k in range(1, n)], "frame", a, o))


if __name__ == "__main__":
    main()
