"""Device time of the chromatic-aberration remap on the C2 shape -- L+R 4096^2 -> 8192 x 4096 side-by-side,
EquirectangularEncoder * PolynomialScaler([0, 1, -0.1]) * FisheyeDecoder("equidistant"), radius "max", bilinear, red =
[0, 1.004, 0, -0.006], blue = [0, 0.997, 0, 0.005] -- by the method of tools/wide_bench.py, next to what it has to beat.

    python tools/chroma_bench.py [--launches 200] [--rounds 3]

Three legs, interleaved and repeated `--rounds` times in one process so that the run-to-run spread is known:

  (a) fused     one v1c_ca_plan_run of two units, as apply_lr_tensors(chromatic=) makes it;
  (b) plain     the uncorrected apply_lr_tensors launch (one v1c_plan_run of two units): the floor;
  (c) split     the only route without the feature: each source split into three contiguous grey planes, three remap_tensors calls
                with the three channel chains on the grey pairs, torch.stack of the planes back into BGR.

Timed with device events over `--launches` launches per leg and round after a warm-up, sources and outputs rotated over more than
640 MiB so that no launch finds its source in the Infinity Cache.  One JSON line per leg: ms per call in every round, their median and
spread (max - min), and the kernel family; a last line with the verdict -- (a) against (c) beyond the larger of the two spreads.

(a) and (b) submit pre-marshalled units, one C call per launch.  (c) goes through `remap_tensors` and torch, as a caller of that route
would; device events only hide its host time while the queue stays full, which six launches of this size per call keep it.  There is
one fused form, the global-memory kernel: no leg with a kernel switched off."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from vr180_convert_amd import chromatic, remapper  # noqa: E402
from vr180_convert_amd.chain import lower_for_get_map  # noqa: E402
from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder, PolynomialScaler  # noqa: E402

RED, BLUE = [0, 1.004, 0, -0.006], [0, 0.997, 0, 0.005]
N = W = 4096


def timed(fn, launches: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(launches):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    t = EquirectangularEncoder() * PolynomialScaler([0, 1, -0.1]) * FisheyeDecoder("equidistant")
    ca = chromatic.ChromaticAberration(red=RED, blue=BLUE)
    tcs = ca.channel_transformers(t)
    kw = dict(radius=N / 2, size_input=(N, N), size_output=(W, N))
    ca_plan = chromatic.CaPlan(chromatic.lower_channels(t, ca, **kw), src_hw=(N, N), dst_wh=(W, N), interpolation=1, border_mode=0,
                               border_value=0, device=dev)
    plain = remapper.Plan(lower_for_get_map(t, **kw), src_hw=(N, N), dst_wh=(W, N), cn=3, interpolation=1, border_mode=0, border_value=0,
                          device=dev)
    pair_bytes = 2 * N * N * 3 + N * 2 * W * 3
    sets = max(2, -(-(640 << 20) // pair_bytes) + 1)  # > 640 MiB in rotation
    bufs = []
    for k in range(sets):
        g = torch.Generator(device=dev).manual_seed(k)
        src = [torch.randint(0, 256, (N, N, 3), generator=g, device=dev, dtype=torch.int32).to(torch.uint8) for _ in range(2)]
        out = torch.empty((N, 2 * W, 3), dtype=torch.uint8, device=dev)
        units = remapper.marshal_units(src, [out[:, :W], out[:, W:]], None, src_hw=(N, N), dst_wh=(W, N), cn=3, device=dev)
        planes_out = torch.empty((3, N, 2 * W, 1), dtype=torch.uint8, device=dev)
        bufs.append({"units": units, "src": src, "out": out, "planes_out": planes_out})

    def leg_fused(k):
        ca_plan.run_units(bufs[k % sets]["units"], 2)  # (pre-marshalled, like the plain leg: the same host work per call)

    def leg_plain(k):
        plain.run_units(bufs[k % sets]["units"], 2)

    def leg_split(k):
        b = bufs[k % sets]
        planes = [s.permute(2, 0, 1).contiguous() for s in b["src"]]  # (3, N, N): three contiguous grey planes per eye
        for c in range(3):
            po = b["planes_out"][c]
            remapper.remap_tensors(tcs[c], [planes[0][c][..., None], planes[1][c][..., None]], [po[:, :W], po[:, W:]], radius=N / 2,
                                   interpolation=1, size_input=(N, N))
        b["out"].copy_(torch.stack([b["planes_out"][c][..., 0] for c in range(3)], dim=-1))

    legs = [("fused", leg_fused, a.launches), ("plain", leg_plain, a.launches), ("split", leg_split, max(10, a.launches // 4))]
    for _, fn, _n in legs:  # warm-up: plans, memoised units, every buffer set touched
        for k in range(2 * sets):
            fn(k)
    torch.cuda.synchronize()
    kinds = {"fused": ca_plan.last_launch(), "plain": plain.last_launch(), "split": "+".join(remapper.last_launch_kinds())}
    ms: dict[str, list[float]] = {name: [] for name, _, _ in legs}
    for _ in range(a.rounds):
        for name, fn, n in legs:
            ms[name].append(timed(fn, n))
    res = {}
    for name, _, n in legs:
        v = ms[name]
        res[name] = {"leg": name, "ms_per_call": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4),
                     "spread_ms": round(max(v) - min(v), 4), "launches_per_round": n, "rounds": a.rounds, "kind": kinds[name],
                     "buffer_sets": sets, "rotated_mib": round(sets * pair_bytes / 2 ** 20)}
        print(json.dumps(res[name]), flush=True)
    spread = max(res["fused"]["spread_ms"], res["split"]["spread_ms"])
    gain = res["split"]["median_ms"] - res["fused"]["median_ms"]
    print(json.dumps({"verdict": "fused beats split beyond the spread" if gain > spread else "fused does NOT beat split beyond the spread",
                      "split_minus_fused_ms": round(gain, 4), "spread_ms": spread,
                      "fused_over_plain": round(res["fused"]["median_ms"] / res["plain"]["median_ms"], 3),
                      "split_over_fused": round(res["split"]["median_ms"] / res["fused"]["median_ms"], 3)}), flush=True)


if __name__ == "__main__":
    main()
