"""JPEG file bytes -> device tensor: the device decoder (jpeg_decode_device.decode_jpeg_tensor) against the path it replaces (Pillow on
the host + the upload of the decoded frame), for the given files or, without any, for tests/golden/ref_docs/test.jpg (2048 x 2048,
4:2:0, one entropy-coded segment) and a 4096 x 4096 4:2:0 quality-95 file written by Pillow from the sphere scene.

For every file the host-only parse is timed by itself (it is part of every call); for every file and every ``--subseq-bits`` value:
``--runs`` calls after a warm-up, each between two device events and inside a host
clock, the synchronisation rounds the call took and the subsequences it ran over; Pillow's decode and the upload three times.  One
JSON line per (file, subseq_bits); ``--out`` appends them to a file.

``--batch N [N ...]``: instead, for every file and N, a batch of N copies through ``decode_jpeg_tensors`` against N single
``decode_jpeg_tensor`` calls in the same process, the two alternating run by run; one JSON line per (file, N) with the times, the
rounds of both and whether the tensors are equal.

``--progressive``: every file is first written again as a progressive file by Pillow (the same quantisation tables and sampling:
``quality="keep"``), and decoded with ``progressive=True``; the JSON line has the scans and the rounds of every scan too.

    python tools/jpeg_decode_bench.py --progressive --out profiles/jpeg_decode_progressive/bench.jsonl
    python tools/jpeg_decode_bench.py --subseq-bits 512 1024 2048 4096 --out profiles/jpeg_decode/bench.jsonl
    python tools/jpeg_decode_bench.py --batch 2 16 64 --out profiles/jpeg_decode_batch/bench.jsonl
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/jpeg_decode_bench.py --runs 2 --device-only     (per-kernel times)
"""
from __future__ import annotations

import argparse
import collections
import io
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def default_files() -> dict:
    import sphere_scene as S
    from PIL import Image

    big = np.kron(S.render(2048), np.ones((2, 2, 1), np.uint8))  # 4096 x 4096: the scene at twice the size
    big = (big.astype(np.int16) + np.random.default_rng(0).integers(-6, 7, big.shape, dtype=np.int16)).clip(0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(big[..., ::-1])).save(b, "JPEG", quality=95, subsampling=2)
    return {"docs_2048": (ROOT / "tests" / "golden" / "ref_docs" / "test.jpg").read_bytes(), "sphere_4096_q95_420": b.getvalue()}


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


def bench_batches(V, files: dict, sizes: list, subseq_bits: list, runs: int, only: set, out_path) -> None:
    for name, data in files.items():
        for n in sizes:
            if only and f"{name}:{n}" not in only:
                continue
            for S in subseq_bits:
                kw = {} if S == 0 else {"subseq_bits": S}
                items = [data] * n
                got = V.decode_jpeg_tensors(items, **kw)  # warm-up of both: code objects, the staging buffer, the memory pool
                rep = V.last_batch_report()
                one = V.decode_jpeg_tensor(data, **kw)
                single_rounds = V.last_decode_report()["rounds"]
                equal = all(torch.equal(g, one) for g in got)
                del got
                torch.cuda.synchronize()
                # Rotation: every run's tensors stay alive until more than twice the 256 MB Infinity Cache has been written since, so no
                # run stores into lines the cache still holds from the run before (the inputs are host bytes, staged anew every call).
                per_run = n * one.numel()
                held = collections.deque(maxlen=max(1, -(-(2 * 256 << 20) // per_run)))
                batch, loop = [], []
                for _ in range(runs):  # (alternating, so that a drift of the clocks meets both alike)
                    r, ev, host = _timed(lambda: V.decode_jpeg_tensors(items, **kw))
                    batch.append((ev, host))
                    held.append(r)
                    r, ev, host = _timed(lambda: [V.decode_jpeg_tensor(d, **kw) for d in items])
                    loop.append((ev, host))
                    held.append(r)
                held.clear()
                line = {"file": name, "bytes": len(data), "shape": list(one.shape), "subseq_bits": S, "batch": n, "runs": runs,
                        "batch_rounds": rep["batch_rounds"], "chunks": rep["chunks"], "loop_rounds": single_rounds * n,
                        "equal_to_single": bool(equal),
                        "batch_events_ms_min_median_max": _spread([b[0] for b in batch]), "batch_host_ms_min_median_max": _spread([b[1] for b in batch]),
                        "loop_events_ms_min_median_max": _spread([b[0] for b in loop]), "loop_host_ms_min_median_max": _spread([b[1] for b in loop])}
                line["loop_over_batch_median_host"] = round(line["loop_host_ms_min_median_max"][1] / line["batch_host_ms_min_median_max"][1], 3)
                line["loop_over_batch_median_events"] = round(line["loop_events_ms_min_median_max"][1] / line["batch_events_ms_min_median_max"][1], 3)
                text = json.dumps(line)
                print(text, flush=True)
                if out_path:
                    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
                    with open(out_path, "a") as f:
                        f.write(text + "\n")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="*", help="JPEG files (default: the docs image and a 4096 x 4096 sphere scene)")
    ap.add_argument("--subseq-bits", type=int, nargs="+", default=[0], help="0: the engine's default")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--device-only", action="store_true", help="skip the host path (profiler runs)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, nargs="+", default=None, help="batch sizes: N copies in one decode_jpeg_tensors call against N single calls")
    ap.add_argument("--progressive", action="store_true", help="the files written again progressive by Pillow, decoded with progressive=True")
    ap.add_argument("--only", nargs="*", default=[], help="with --batch: only these file:N pairs (docs_2048:64 ...)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_decode_bench needs the MI355X")
    from PIL import Image

    import vr180_convert_amd as V

    dev = torch.device("cuda", 0)
    files = {Path(f).name: Path(f).read_bytes() for f in a.files} if a.files else default_files()
    dkw = {}
    if a.progressive:
        if a.batch:
            raise SystemExit("--progressive has no batch: decode_jpeg_tensors refuses progressive files")
        for name in list(files):
            b = io.BytesIO()
            Image.open(io.BytesIO(files.pop(name))).save(b, "JPEG", quality="keep", subsampling="keep", progressive=True)
            files[name + "_progressive"] = b.getvalue()
        dkw = {"progressive": True}
    if a.batch:
        bench_batches(V, files, a.batch, a.subseq_bits, a.runs, set(a.only), a.out)
        return
    for name, data in files.items():
        host = []
        ref = None
        for _ in range(0 if a.device_only else 3):
            t0 = time.perf_counter()
            arr = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])
            t1 = time.perf_counter()
            torch.from_numpy(arr).to(dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host.append({"decode_ms": 1e3 * (t1 - t0), "upload_ms": 1e3 * (t2 - t1), "total_ms": 1e3 * (t2 - t0)})
            ref = arr
        # the host-only parse by itself (markers and the memchr walk over the scan): it runs twice per decode_jpeg_tensor call, once to
        # size the tensor and once inside v1c_jpeg_decode, and both lie inside host_ms below
        from vr180_convert_amd import jpeg_decode_device as J

        parse = []
        for _ in range(max(a.runs, 3)):
            t0 = time.perf_counter()
            (J.probe_progressive if a.progressive else J.probe)(data)
            parse.append(1e3 * (time.perf_counter() - t0))
        parse.sort()
        for S in a.subseq_bits:
            kw = {**dkw} if S == 0 else {"subseq_bits": S, **dkw}
            out = V.decode_jpeg_tensor(data, **kw)  # warm-up: code objects, the staging buffer, the memory pool
            torch.cuda.synchronize()
            rep = V.last_decode_report()
            runs = []
            for _ in range(a.runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                out = V.decode_jpeg_tensor(data, **kw)
                e1.record()
                e1.synchronize()
                runs.append({"events_ms": e0.elapsed_time(e1), "host_ms": 1e3 * (time.perf_counter() - t0)})
            ev = sorted(r["events_ms"] for r in runs)
            h, w = int(out.shape[0]), int(out.shape[1])
            line = {"file": name, "bytes": len(data), "shape": [h, w, 3], "subseq_bits": S, "runs": a.runs, **rep,
                    "host_parse_ms_min_median": [round(parse[0], 4), round(parse[len(parse) // 2], 4)],
                    "equals_pillow": None if ref is None else bool(np.array_equal(out.cpu().numpy(), ref)),
                    "events_ms_min_median_max": [round(ev[0], 3), round(ev[len(ev) // 2], 3), round(ev[-1], 3)],
                    "mpixel_per_s_median": round(h * w / 1e3 / ev[len(ev) // 2], 1), "device": runs, "host": host}
            text = json.dumps(line)
            print(text, flush=True)
            if a.out:
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(text + "\n")


if __name__ == "__main__":
    main()
