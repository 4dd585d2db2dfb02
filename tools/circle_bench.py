"""Device time of the image-circle fit (``fit_circle_tensor``: four launches, no synchronisation) on uint8 BGR noise discs of
2048 x 2048, 4096 x 4096 and 8192 x 4096, against its upper bound: the work reads the image at most twice, so two ``torch.clone`` of
the image, timed in the same run, are the yardstick.

``--runs`` calls (at least 200) after a warm-up, over ``--buffers`` rotating copies of the image (as bench.py rotates its buffers: the
copies together exceed the last-level cache), each call between two device events; the clones alternate with the fits, call by call.
One JSON line per size and kind of frame (``disc``: the circle touches the frame; ``small``: a disc of a quarter of the height in a
black frame, where the scans read almost everything); ``--out`` appends them to a file.

    python tools/circle_bench.py --out profiles/circle_fit/bench.jsonl
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/circle_bench.py --runs 200 --sizes 4096x4096     (per-kernel times)
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT)]


def frame(h: int, w: int, kind: str, dev: torch.device, seed: int) -> torch.Tensor:
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    img = torch.randint(40, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=g)
    r = min(h, w) / 2 if kind == "disc" else min(h, w) / 4
    yy = torch.arange(h, device=dev, dtype=torch.float32)[:, None] - (h / 2 - 0.5)
    xx = torch.arange(w, device=dev, dtype=torch.float32)[None, :] - (w / 2 - 0.5)
    img[(xx * xx + yy * yy) > r * r] = 0
    return img


def _mmm(v: list[float]) -> list[float]:
    v = sorted(v)
    return [round(v[0], 4), round(v[len(v) // 2], 4), round(v[-1], 4)]


def main() -> int:
    import vr180_convert_amd as V

    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--buffers", type=int, default=6)
    ap.add_argument("--sizes", nargs="+", default=["2048x2048", "4096x4096", "8192x4096"], help="WxH")
    ap.add_argument("--kinds", nargs="+", default=["disc", "small"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for size in a.sizes:
        w, h = (int(v) for v in size.split("x"))
        for kind in a.kinds:
            bufs = [frame(h, w, kind, dev, k) for k in range(a.buffers)]
            for b in bufs[:2]:  # warm-up: code objects, the memory pool
                V.fit_circle_tensor(b)
                b.clone().clone()
            torch.cuda.synchronize()
            fit_ms, clone_ms, outs = [], [], []
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            for k in range(a.runs):
                b = bufs[k % len(bufs)]
                ev[0].record()
                outs.append(V.fit_circle_tensor(b))
                ev[1].record()
                c = b.clone().clone()
                ev[2].record()
                ev[2].synchronize()
                fit_ms.append(ev[0].elapsed_time(ev[1]))
                clone_ms.append(ev[1].elapsed_time(ev[2]))
                del c
            res = torch.stack(outs[: len(bufs)]).cpu().numpy()
            line = {"size": size, "frame": kind, "dtype": "uint8", "cn": 3, "runs": a.runs, "buffers": len(bufs),
                    "fit_ms_min_median_max": _mmm(fit_ms), "two_clones_ms_min_median_max": _mmm(clone_ms),
                    "fit_over_two_clones_median": round(_mmm(fit_ms)[1] / _mmm(clone_ms)[1], 3),
                    "first_result": [round(float(v), 4) for v in res[0]], "status_all_zero": bool((res[:, 3] == 0).all())}
            print(json.dumps(line), flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
            del bufs
    return 0


if __name__ == "__main__":
    sys.exit(main())
