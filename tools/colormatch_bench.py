"""Device time of the colour match of two eyes (``color_match_luts_tensor`` + ``apply_luts_tensor``: four launches, no
synchronisation) on uint8 BGR pairs of 2048 x 2048 and 4096 x 4096 per eye, on noise and on a flat frame (every lane on one bin: the
histogram's worst case), against a torch composition of the same step: ``torch.bincount`` per channel over the masked pixels of both
eyes, the table rule on the host (NumPy, the restatement's), ``lut[img.long()]``.

``--runs`` calls (at least 200) after a warm-up, over ``--buffers`` rotating pairs (as bench.py rotates its buffers: the pairs together
exceed the last-level cache), each part between two device events: the chain, the tables alone (``k_cm_zero``, ``k_cm_hist``, ``k_cm_luts``) and
the apply alone (``k_cm_apply``).  The histogram pass reads both eyes once; its share of the HBM bandwidth (``--hbm-gbs``, 8000 by
default) stands next to its time.  The torch composition synchronises (the tables are built on the host), so it is timed on the host
clock around a synchronisation, ``--baseline-runs`` times.  One JSON line per size and content; ``--out`` appends them to a file.

    python tools/colormatch_bench.py --out profiles/colormatch/bench.jsonl
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/colormatch_bench.py --runs 200 --sizes 4096x4096 --baseline-runs 0
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def pair(h: int, w: int, kind: str, dev: torch.device, seed: int):
    if kind == "flat":
        return torch.full((h, w, 3), 100, dtype=torch.uint8, device=dev), torch.full((h, w, 3), 125, dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    left = torch.randint(10, 181, (h, w, 3), dtype=torch.uint8, device=dev, generator=g)
    return left, left + (left >> 2)


def torch_composition(left: torch.Tensor, right: torch.Tensor, mode: str) -> torch.Tensor:
    """the same step with torch operators and the table rule on the host; returns the rewritten right eye"""
    import colormatch_ref as R

    ml, mr = left.amax(dim=2), right.amax(dim=2)
    m = (ml >= 10) & (ml <= 254) & (mr >= 10) & (mr <= 254)
    hist = torch.stack([torch.stack([torch.bincount(e[..., c][m].long(), minlength=256) for c in range(3)]) for e in (left, right)]).cpu().numpy()
    luts = np.stack([R.histogram_lut(hist[1, c], hist[0, c]) if mode == "histogram" else R.gain_lut(R.gain_of(hist[1, c], hist[0, c]) or 65536)
                     for c in range(3)])
    lut = torch.from_numpy(luts).to(left.device)
    return torch.stack([lut[c][right[..., c].long()] for c in range(3)], dim=2)


def _mmm(v: list[float]) -> list[float]:
    v = sorted(v)
    return [round(v[0], 4), round(v[len(v) // 2], 4), round(v[-1], 4)] if v else []


def main() -> int:
    from vr180_convert_amd import colormatch

    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--baseline-runs", type=int, default=10)
    ap.add_argument("--buffers", type=int, default=6)
    ap.add_argument("--sizes", nargs="+", default=["2048x2048", "4096x4096"], help="WxH per eye")
    ap.add_argument("--kinds", nargs="+", default=["noise", "flat"])
    ap.add_argument("--modes", nargs="+", default=["histogram"])
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM bandwidth the histogram pass is set against")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for size in a.sizes:
        w, h = (int(v) for v in size.split("x"))
        for kind in a.kinds:
            for mode in a.modes:
                bufs = [pair(h, w, kind, dev, k) for k in range(a.buffers)]
                outs = [torch.empty_like(b[1]) for b in bufs]
                ws = torch.empty((2, 3, 256), dtype=torch.int32, device=dev)
                for (l, r), o in zip(bufs[:2], outs):  # warm-up: code objects, the memory pool
                    luts, _ = colormatch.color_match_luts_tensor(l, r, workspace=ws, mode=mode)
                    colormatch.apply_luts_tensor(r, luts, out=o)
                torch.cuda.synchronize()
                luts_ms, apply_ms, chain_ms = [], [], []
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                for k in range(a.runs):
                    (l, r), o = bufs[k % len(bufs)], outs[k % len(bufs)]
                    ev[0].record()
                    luts, report = colormatch.color_match_luts_tensor(l, r, workspace=ws, mode=mode)
                    ev[1].record()
                    colormatch.apply_luts_tensor(r, luts, out=o)
                    ev[2].record()
                    ev[2].synchronize()
                    luts_ms.append(ev[0].elapsed_time(ev[1]))
                    apply_ms.append(ev[1].elapsed_time(ev[2]))
                    chain_ms.append(ev[0].elapsed_time(ev[2]))
                base_ms = []
                same = None
                for k in range(a.baseline_runs + 1):
                    l, r = bufs[k % len(bufs)]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    want = torch_composition(l, r, mode)
                    torch.cuda.synchronize()
                    if k:  # (the first call warms torch's own kernels up)
                        base_ms.append((time.perf_counter() - t0) * 1e3)
                    else:
                        luts, _ = colormatch.color_match_luts_tensor(l, r, workspace=ws, mode=mode)
                        same = bool(torch.equal(colormatch.apply_luts_tensor(r, luts), want))
                read_bytes = 2 * h * w * 3
                med = _mmm(luts_ms)[1]
                line = {"size_per_eye": size, "content": kind, "mode": mode, "runs": a.runs, "buffers": len(bufs),
                        "chain_ms_min_median_max": _mmm(chain_ms), "luts_ms_min_median_max": _mmm(luts_ms),
                        "apply_ms_min_median_max": _mmm(apply_ms), "hist_read_MB": round(read_bytes / 1e6, 1),
                        "luts_pass_GBs_median": round(read_bytes / med / 1e6, 1), "luts_pass_share_of_hbm": round(read_bytes / med / 1e6 / a.hbm_gbs, 3),
                        "apply_GBs_median": round(2 * h * w * 3 / _mmm(apply_ms)[1] / 1e6, 1),
                        "torch_composition_ms_min_median_max": _mmm(base_ms), "status": int(report[0].item()),
                        "equals_torch_composition": same}
                if base_ms:
                    line["torch_over_chain_median"] = round(_mmm(base_ms)[1] / _mmm(chain_ms)[1], 1)
                print(json.dumps(line), flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(json.dumps(line) + "\n")
                del bufs, outs
    return 0


if __name__ == "__main__":
    sys.exit(main())
