"""Device time of the 16-bit / float32 remap (k_remap_wide) on the C2 shape -- L+R 4096^2 -> 8192 x 4096 side-by-side,
EquirectangularEncoder * PolynomialScaler([0, 1, -0.1]) * FisheyeDecoder("equidistant"), radius "max" -- next to 8-bit.

    python tools/wide_bench.py [--launches 200] [--interp 1 4] [--types u8 u16 f32]

One launch = both eyes (one v1c_plan_run of two units, as apply_lr_tensors makes it).  Timed with device events over `--launches`
launches after a warm-up, the inputs and outputs rotated over more than 512 MiB so that no launch finds its source in the Infinity
Cache.  Prints one JSON line per (type, interpolation): ms per launch and the kernel family the plan used.  For the 8-bit generic kernel
run it against the tuning build with the fast kernels off: V1C_LIB=vr180_convert_amd/csrc/libvr180remap_tuning.so
V1C_DISABLE_FAST=1."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from vr180_convert_amd import remapper  # noqa: E402
from vr180_convert_amd.chain import lower_for_get_map  # noqa: E402
from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder, PolynomialScaler  # noqa: E402

TYPES = {"u8": torch.uint8, "u16": torch.uint16, "f32": torch.float32}


def one(kind: str, interp: int, launches: int, dev: torch.device) -> dict:
    dtype = TYPES[kind]
    n, w = 4096, 4096
    t = EquirectangularEncoder() * PolynomialScaler([0, 1, -0.1]) * FisheyeDecoder("equidistant")
    chain = lower_for_get_map(t, radius=n / 2, size_input=(n, n), size_output=(w, n))
    plan = remapper.Plan(chain, src_hw=(n, n), dst_wh=(w, n), cn=3, interpolation=interp, border_mode=0, border_value=0, device=dev,
                         dtype=dtype)
    esz = torch.empty((), dtype=dtype).element_size()
    pair_bytes = 2 * n * n * 3 * esz + n * 2 * w * 3 * esz
    sets = max(2, -(-(600 << 20) // pair_bytes))  # > 512 MiB in rotation
    bufs = []
    for k in range(sets):
        g = torch.Generator(device=dev).manual_seed(k)
        if dtype == torch.float32:
            src = [torch.rand((n, n, 3), generator=g, device=dev) for _ in range(2)]
        else:
            hi = 256 if dtype == torch.uint8 else 65536
            src = [torch.randint(0, hi, (n, n, 3), generator=g, device=dev, dtype=torch.int32).to(dtype) for _ in range(2)]
        out = torch.empty((n, 2 * w, 3), dtype=dtype, device=dev)
        units = remapper.marshal_units(src, [out[:, :w], out[:, w:]], None, src_hw=(n, n), dst_wh=(w, n), cn=3, device=dev, dtype=dtype)
        bufs.append((units, src, out))
    for k in range(2 * sets):
        plan.run_units(bufs[k % sets][0], 2)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(launches):
        plan.run_units(bufs[k % sets][0], 2)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / launches
    return {"type": kind, "interp": interp, "ms_per_launch": round(ms, 4), "launches": launches, "buffer_sets": sets,
            "rotated_mib": round(sets * pair_bytes / 2 ** 20), "kind": plan.last_launch(),
            "gb_per_s_pixels": round(pair_bytes / (ms * 1e-3) / 1e9, 1)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--interp", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--types", nargs="+", default=["u8", "u16", "f32"], choices=list(TYPES))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for kind in a.types:
        for interp in a.interp:
            print(json.dumps(one(kind, interp, a.launches, dev)), flush=True)


if __name__ == "__main__":
    main()
