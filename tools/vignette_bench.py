"""Device time of the vignetting correction (``apply_vignette_tensor``: one launch; ``vignette_rings_tensor``: two) on BGR frames of
2048 x 2048 and 4096 x 4096 per eye, uint8 and uint16, next to what it has to be read against:

  (a) ``k_vig_apply`` (``apply_vignette_tensor`` with resident tables),
  (b) a device copy of the same tensor (``out.copy_(img)``): the floor of a pass that reads once and writes once,
  (c) the torch composition a user would write today: a precomputed float32 gain map of the frame's shape, multiply, round, clamp, cast,
  (d) the ring statistics on noise and on a flat frame (every lane of a wave in one ring: the merge's best case, the atomics' worst),
  (e) a C2-shaped ``apply_lr_tensors`` (L+R -> side by side at the frame's size, PolynomialScaler, bilinear, radius "max") with and
      without ``vignette=``.

``--runs`` calls (at least 200) after a warm-up, over ``--buffers`` rotating frames (as bench.py rotates its buffers: together they
exceed the last-level cache), the legs INTERLEAVED inside every run, each between two device events on one stream; minimum, median and
maximum per leg.  One JSON line per size and type; ``--out`` appends them to a file.

    python tools/vignette_bench.py --out profiles/vignette/bench.jsonl
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/vignette_bench.py --runs 50 --sizes 4096x4096 --legs a d
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

COEFS = (-0.35, -0.2, 0.05)  # about one and a half stops at the rim


def _mmm(v: list[float]) -> list[float]:
    v = sorted(v)
    return [round(v[0], 4), round(v[len(v) // 2], 4), round(v[-1], 4)] if v else []


def frame(h: int, w: int, dtype, seed: int, dev) -> torch.Tensor:
    top = 255 if dtype == np.uint8 else 65535
    return torch.from_numpy(np.random.default_rng(seed).integers(top // 25, top * 3 // 4, (h, w, 3), dtype=dtype)).to(dev)


def main() -> int:
    import vr180_convert_amd as V
    from vr180_convert_amd import vignette as VG
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder, PolynomialScaler

    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--buffers", type=int, default=6)
    ap.add_argument("--sizes", nargs="+", default=["2048x2048", "4096x4096"], help="WxH per eye")
    ap.add_argument("--types", nargs="+", default=["uint8", "uint16"])
    ap.add_argument("--legs", nargs="+", default=["a", "b", "c", "d", "e"])
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM bandwidth the gain pass is set against")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    v = VG.Vignette(COEFS)
    chain = EquirectangularEncoder() * PolynomialScaler([0, 1, -0.1]) * FisheyeDecoder("equidistant")
    for size in a.sizes:
        w, h = (int(q) for q in size.split("x"))
        radius = min(h, w) / 2
        for tname in a.types:
            dtype = np.uint8 if tname == "uint8" else np.uint16
            top = 255 if dtype == np.uint8 else 65535
            bufs = [frame(h, w, dtype, k, dev) for k in range(a.buffers)]
            outs = [torch.empty_like(b) for b in bufs]
            flat = torch.from_numpy(np.full((h, w, 3), top // 2, dtype)).to(dev)
            tables = VG.tables_tensor(v, dev)
            gmap = None
            if "c" in a.legs:
                yy, xx = np.mgrid[0:h, 0:w]
                rho2 = ((xx - w // 2) ** 2 + (yy - h // 2) ** 2) / radius ** 2
                gmap = torch.from_numpy(np.ascontiguousarray(np.moveaxis(v.gain(rho2), 0, 2).astype(np.float32))).to(dev)
            sbs = torch.empty((h, 2 * w, 3), dtype=bufs[0].dtype, device=dev) if "e" in a.legs else None

            def leg_a(k):
                VG.apply_vignette_tensor(bufs[k], None, radius=radius, out=outs[k], tables=tables)

            def leg_b(k):
                outs[k].copy_(bufs[k])

            def leg_c(k):
                return (bufs[k].to(torch.float32) * gmap).round_().clamp_(0, top).to(bufs[k].dtype)

            def leg_d_noise(k):
                VG.vignette_rings_tensor(bufs[k], radius=radius, rings=256)

            def leg_d_flat(k):
                VG.vignette_rings_tensor(flat, radius=radius, rings=256)

            def leg_e_plain(k):
                V.apply_lr_tensors(chain, bufs[k], bufs[(k + 1) % len(bufs)], out=sbs, size_output=(w, h), interpolation=1, radius="max")

            def leg_e_vig(k):
                V.apply_lr_tensors(chain, bufs[k], bufs[(k + 1) % len(bufs)], out=sbs, size_output=(w, h), interpolation=1, radius="max", vignette=v)

            legs = [(n, f) for n, f, key in (("a_apply", leg_a, "a"), ("b_copy", leg_b, "b"), ("c_torch", leg_c, "c"),
                                             ("d_rings_noise", leg_d_noise, "d"), ("d_rings_flat", leg_d_flat, "d"),
                                             ("e_apply_lr", leg_e_plain, "e"), ("e_apply_lr_vignette", leg_e_vig, "e")) if key in a.legs]
            skipped = {}
            for n, f in list(legs):  # warm-up: code objects, plans, the memory pool; a leg torch cannot run for this type is left out
                try:
                    for k in range(2):
                        f(k)
                    torch.cuda.synchronize()
                except (RuntimeError, NotImplementedError, TypeError) as e:
                    skipped[n] = str(e).splitlines()[0][:120]
                    legs = [q for q in legs if q[0] != n]
            same = None
            if "c" in a.legs and "c_torch" not in skipped:
                leg_a(0)
                diff = (leg_c(0).to(torch.int32) - outs[0].to(torch.int32)).abs().max().item()
                same = int(diff)
            ms = {n: [] for n, _ in legs}
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(legs) + 1)]
            for r in range(a.runs):
                k = r % len(bufs)
                ev[0].record()
                for i, (n, f) in enumerate(legs):
                    f(k)
                    ev[i + 1].record()
                ev[-1].synchronize()
                for i, (n, _) in enumerate(legs):
                    ms[n].append(ev[i].elapsed_time(ev[i + 1]))
            nbytes = h * w * 3 * bufs[0].element_size()
            line = {"size_per_eye": size, "type": tname, "runs": a.runs, "buffers": len(bufs), "frame_MB": round(nbytes / 1e6, 1),
                    **{f"{n}_ms_min_median_max": _mmm(t) for n, t in ms.items()}, "skipped": skipped,
                    "torch_composition_largest_difference_levels": same}
            if "a_apply" in ms:
                med = _mmm(ms["a_apply"])[1]
                line["a_apply_GBs_median"] = round(2 * nbytes / med / 1e6, 1)
                line["a_apply_share_of_hbm"] = round(2 * nbytes / med / 1e6 / a.hbm_gbs, 3)
                if "b_copy" in ms:
                    line["a_over_b_median"] = round(med / _mmm(ms["b_copy"])[1], 2)
                if "c_torch" in ms:
                    line["c_over_a_median"] = round(_mmm(ms["c_torch"])[1] / med, 1)
            if "e_apply_lr" in ms and "e_apply_lr_vignette" in ms:
                line["e_vignette_adds_ms_median"] = round(_mmm(ms["e_apply_lr_vignette"])[1] - _mmm(ms["e_apply_lr"])[1], 4)
            print(json.dumps(line), flush=True)
            if a.out:
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
            del bufs, outs, flat, gmap, sbs
    return 0


if __name__ == "__main__":
    sys.exit(main())
