"""Device tensor -> PNG bytes on the host: the device encoder (png_device.encode_png_tensor) against the path it replaces
(``t.cpu().numpy()`` + ``_png.encode(level=1, threads=16)``), on a C2-sized side-by-side result (8192 x 4096 x 3).

Two images: the remap of a sphere-scene pair (drawn content) and of a noise-disc pair (the incompressible extreme).  The two paths
alternate in one session, ``--runs`` each after a warm-up, over rotated copies of the result (as bench.py rotates its buffers).  Every
time is a host clock around work that ends in a device synchronisation.  One JSON line per image; ``--out`` appends them to a file.

    python tools/png_device_bench.py --out profiles/png_device/bench.jsonl
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/png_device_bench.py --runs 2 --device-only     (per-kernel times)
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


def results(size: int, dev: torch.device) -> dict:
    import sphere_scene as S
    import vr180_convert_amd as V
    from vr180_convert_amd.synth import noise_disc
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder

    t = EquirectangularEncoder() * FisheyeDecoder("equidistant")
    src = min(size, 2048)
    pairs = {"sphere": (S.render(src), S.render(src, S.rotation([0.3, 1, 0.2], 4))), "noise_disc": (noise_disc(size, size, 0), noise_disc(size, size, 1))}
    out = {}
    for name, (left, right) in pairs.items():
        out[name] = V.apply_lr_tensors(t, torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev), size_output=(size, size),
                                       interpolation=1, radius="max")
    torch.cuda.synchronize()
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=4096, help="output size per eye")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="threads of the host writer")
    ap.add_argument("--filter", default="up")
    ap.add_argument("--device-only", action="store_true", help="skip the host path (profiler runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("png_device_bench needs the MI355X")
    from vr180_convert_amd import _png, png_device as P

    dev = torch.device("cuda", 0)
    for name, sbs in results(a.size, dev).items():
        copies = [sbs.clone() for _ in range(3)]
        h, w, cn = (int(v) for v in sbs.shape)

        def device_path(t):
            t0 = time.perf_counter()
            segs, bands = P.deflate_tensor(t, filter=a.filter)  # the ABI call: kernels, the codes on the host, the copy of the stream
            t1 = time.perf_counter()
            png = _png.assemble(segs, [b[:5] for b in bands], width=w, height=h, channels=cn, filter_type=P.FILTERS[a.filter], threads=a.threads)
            t2 = time.perf_counter()
            return png, {"deflate_call_ms": 1e3 * (t1 - t0), "crc_assemble_ms": 1e3 * (t2 - t1), "total_ms": 1e3 * (t2 - t0),
                         "stored_bands": sum(b[5] for b in bands), "bands": len(bands)}

        def host_path(t):
            t0 = time.perf_counter()
            host = t.cpu().numpy()
            t1 = time.perf_counter()
            png = _png.encode(host, level=1, threads=a.threads)
            t2 = time.perf_counter()
            return png, {"copy_ms": 1e3 * (t1 - t0), "filter_deflate_ms": 1e3 * (t2 - t1), "total_ms": 1e3 * (t2 - t0)}

        png_d, _ = device_path(copies[0])  # warm-up: code objects, the page-locked buffer, the memory pool
        png_h = None if a.device_only else host_path(copies[0])[0]
        torch.cuda.synchronize()
        drun, hrun = [], []
        for k in range(a.runs):
            t = copies[k % 3]
            drun.append(device_path(t)[1])
            if not a.device_only:
                hrun.append(host_path(t)[1])
        own = _png.decode(png_d)
        line = {"image": name, "shape": [h, w, cn], "filter": a.filter, "runs": a.runs, "threads": a.threads, "raw_bytes": h * w * cn,
                "device_png_bytes": len(png_d), "host_png_bytes": None if png_h is None else len(png_h),
                "size_ratio": None if png_h is None else round(len(png_d) / len(png_h), 4),
                "decodes_to_input": bool(own is not None and np.array_equal(own, sbs.cpu().numpy())),
                "device": drun, "host": hrun,
                "every_device_run_faster": None if not hrun else max(r["total_ms"] for r in drun) < min(r["total_ms"] for r in hrun)}
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
