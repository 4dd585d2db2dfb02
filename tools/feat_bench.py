"""Device time per stage of the feature pipeline (--automatch devfm) on a 4096^2 BGR sphere-scene pair, at s = 1 and s = 0.5, plus the
keypoint and match counts.

    python tools/feat_bench.py [--runs 20] [--n 4096]

Each stage kernel of v1c_feat_detect / v1c_feat_match is timed as a whole call bracketed by device events (detect of one eye, match of
the pair), averaged over `--runs` after a warm-up; the per-kernel split comes from `rocprofv3 --kernel-trace --stats` of the same script.
Prints one JSON line per scale."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))

import sphere_scene as S  # noqa: E402
from vr180_convert_amd import features as F  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--n", type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rot = S.rotation([1, 0, 0], 3) @ S.rotation([0, 1, 0], 2)
    left = torch.from_numpy(S.render(args.n)).to(dev)
    right = torch.from_numpy(S.render(args.n, rot)).to(dev)
    for scale in (1.0, 0.5):
        p = F.params(scale, args.n / 2)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        det_ms = match_ms = 0.0
        for k in range(args.runs + 2):
            e[0].record()
            kp1, d1, c1 = F._detect_enqueue(left, p)
            e[1].record()
            kp2, d2, c2 = F._detect_enqueue(right, p)
            n1, n2 = (int(v) for v in torch.cat([c1, c2]).cpu())
            e[2].record()
            pairs, dist, cm = F._match_enqueue(d1[:n1], d2[:n2], p)
            e[3].record()
            torch.cuda.synchronize()
            if k >= 2:
                det_ms += e[0].elapsed_time(e[1]) / args.runs
                match_ms += e[2].elapsed_time(e[3]) / args.runs
        print(json.dumps({"n": args.n, "scale": scale, "detect_ms_per_eye": round(det_ms, 4), "match_ms": round(match_ms, 4),
                          "keypoints": [n1, n2], "matches": int(cm.item()), "runs": args.runs}), flush=True)


if __name__ == "__main__":
    main()
