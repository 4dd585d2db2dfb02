#!/usr/bin/env python3
"""Static instruction-class counts of the project's mirror kernels, per barrier segment.

    python3 tools/static_counts.py [OBJECT ...] [--kernel SUBSTRING ...]

Disassembles the gfx950 code object inside each OBJECT (default: vr180_convert_amd/csrc/kernels_mirror.o) with llvm-objdump and
prints, for every kernel whose mangled name contains one of the substrings (default: the <1, 0> and <0, 1> instantiations of
k_ray_lin3_pair_mirror_seq), the number of VALU (fp64 separately), SALU, SMEM, LDS, LDS-DMA, vector load and store instructions in
each segment of the text: segment 0 runs up to the first LDS-DMA request of a box (the SGPR-base form behind an M0 write), the next
ones end at each s_barrier, in address order.  Both sides of a branch are in the text, so these are static counts, not executed
ones (the wait tables' 21 blocks count as one wait).  Registers and LDS come from the code object's metadata notes.

Evidence for profiles/*/static_counts.txt; nothing asserts these numbers."""
from __future__ import annotations

import argparse
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
OBJDUMP = Path("/opt/rocm/lib/llvm/bin/llvm-objdump")
READELF = Path("/opt/rocm/lib/llvm/bin/llvm-readelf")
CLASSES = ("VALU", "fp64", "qrate", "SALU", "SMEM", "LDS", "DMA", "VLOAD", "STORE")
QUARTER = ("v_mul_lo_u32", "v_mul_hi_u32", "v_rcp_", "v_rsq_", "v_sqrt_", "v_mul_hi_i32")


def classify(op: str) -> list[str]:
    if op.startswith("global_load_lds"):
        return ["DMA"]
    if re.match(r"(global|buffer|flat|scratch)_load", op):
        return ["VLOAD"]
    if re.match(r"(global|buffer|flat|scratch)_(store|atomic)", op):
        return ["STORE"]
    if op.startswith("ds_"):
        return ["LDS"]
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return ["SMEM"]
    if op.startswith("v_"):
        out = ["VALU"]
        if "f64" in op:
            out.append("fp64")
        if op.startswith(QUARTER):
            out.append("qrate")
        return out
    if op.startswith("s_") and op not in ("s_nop", "s_waitcnt", "s_barrier", "s_endpgm", "s_code_end"):
        return ["SALU"]
    return []


def code_object(obj: Path, work: Path) -> Path:
    shutil.copy(obj, work / "k.o")
    subprocess.run([str(OBJDUMP), "--offloading", "k.o"], cwd=work, check=True, capture_output=True)
    code = [p for p in work.iterdir() if "gfx950" in p.name]
    assert len(code) == 1, [p.name for p in work.iterdir()]
    return code[0]


def kernels(code: Path) -> dict[str, list[tuple[str, str]]]:
    r = subprocess.run([str(OBJDUMP), "-d", "--no-show-raw-insn", code.name], cwd=code.parent, check=True, capture_output=True, text=True)
    out: dict[str, list[tuple[str, str]]] = {}
    cur = None
    for line in r.stdout.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s*(\S+)\s*(.*?)\s*//\s*[0-9A-Fa-f]+:", line)
        if m and cur is not None:
            cur.append((m.group(1), m.group(2)))
    return out


def registers(code: Path) -> dict[str, tuple[int, int, int]]:
    r = subprocess.run([str(READELF), "--notes", code.name], cwd=code.parent, check=True, capture_output=True, text=True)
    out, name, vals = {}, None, {}
    for line in r.stdout.splitlines():
        m = re.match(r"\s*\.?(name|vgpr_count|sgpr_count|group_segment_fixed_size):\s*(\S+)", line.replace("- ", "  "))
        if not m:
            continue
        if m.group(1) == "name" and not m.group(2).endswith(".kd") and m.group(2).startswith("_Z"):
            name = m.group(2)
        elif m.group(1) != "name":
            vals[m.group(1)] = int(m.group(2))
        if name and len(vals) == 3:
            out[name] = (vals["vgpr_count"], vals["sgpr_count"], vals["group_segment_fixed_size"])
            name, vals = None, {}
    return out


def segments(ins: list[tuple[str, str]]) -> list[dict[str, int]]:
    segs = [dict.fromkeys(CLASSES, 0)]
    seen_box = False
    in_table = 0
    for i, (op, args) in enumerate(ins):
        if in_table:  # the other 20 blocks of a wait table
            in_table -= 1
            continue
        if op == "s_setpc_b64" and args.strip() == "vcc":
            segs.append(dict.fromkeys(CLASSES, 0))  # the wait's barrier ends the segment
            in_table = 21 * 4 - 1
            continue
        if not seen_box and op == "global_load_lds_dwordx4" and i >= 2 and ins[i - 2][0] == "s_mov_b32" and ins[i - 2][1].startswith("m0"):
            seen_box = True
            segs.append(dict.fromkeys(CLASSES, 0))
        if op == "s_barrier":
            segs.append(dict.fromkeys(CLASSES, 0))
            continue
        for c in classify(op):
            segs[-1][c] += 1
    return segs


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("objects", nargs="*", default=[str(ROOT / "vr180_convert_amd/csrc/kernels_mirror.o")])
    ap.add_argument("--kernel", action="append", default=None)
    a = ap.parse_args()
    pats = a.kernel or ["k_ray_lin3_pair_mirror_seqILi1ELi0EE", "k_ray_lin3_pair_mirror_seqILi0ELi1EE"]
    for obj in a.objects:
        with tempfile.TemporaryDirectory() as d:
            code = code_object(Path(obj), Path(d))
            dis, regs = kernels(code), registers(code)
            for name, ins in sorted(dis.items()):
                if not any(p in name for p in pats):
                    continue
                segs = segments(ins)
                print(f"== {obj}\n   {name}")
                if name in regs:
                    print("   VGPRs %d  SGPRs %d  static LDS %d B" % regs[name])
                print("   %-28s" % "segment" + "".join("%7s" % c for c in CLASSES))
                labels = ["to first box request"] + ["to barrier %d" % k for k in range(1, len(segs))]
                labels[-1] = "to end"
                for lab, s in zip(labels, segs):
                    print("   %-28s" % lab + "".join("%7d" % s[c] for c in CLASSES))
                tot = {c: sum(s[c] for s in segs) for c in CLASSES}
                print("   %-28s" % "total" + "".join("%7d" % tot[c] for c in CLASSES))
    return 0


if __name__ == "__main__":
    sys.exit(main())
