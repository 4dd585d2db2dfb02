"""What the length of the stall of tests/stream_order.py rests on: its calibration, and the host time of every launch-only call of
tests/test_gpu_stream_order*.py, warm, at the tests' shapes (profiles/stream_order/call_times.txt).  Run on the GPU box:

    python tools/stream_order_times.py
"""
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import analytic_ref as A  # noqa: E402
import chainspecs as CS  # noqa: E402
import circle_cases as CC  # noqa: E402
import stream_order as SO  # noqa: E402
import vr180_convert_amd as V  # noqa: E402
from test_analytic_remap import BV, PLAIN, WIDE_PLAIN, noise_case  # noqa: E402
from test_gpu_analytic import C0, EQUI  # noqa: E402
from test_gpu_codec_threads import feature_pair  # noqa: E402
from test_gpu_mirror_record import PAIR_CASES, frames  # noqa: E402
from test_gpu_parity import LEAN_BATCH  # noqa: E402
from vr180_convert_amd import _native, circle, features as F, remapper as R  # noqa: E402
from vr180_convert_amd.chain import lower_for_get_map  # noqa: E402

ROWS: list = []


def timed(stream, label, fn, n=7):
    """fn() twice to warm up, then n times with the stream idle: the wall-clock time of the call alone"""
    with torch.cuda.stream(stream):
        fn()
        fn()
        stream.synchronize()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
            stream.synchronize()
    ROWS.append((label, statistics.median(ts), max(ts)))
    print(f"{label:42s} median {statistics.median(ts):7.3f} ms   max {max(ts):7.3f} ms", flush=True)


def units(spec, imgs, out_wh, radius, interp, bv, rots=None, dt=torch.uint8):
    srcs = [SO.up(i) for i in imgs]
    dsts = [torch.empty((out_wh[1], out_wh[0], imgs[0].shape[2]), dtype=dt, device="cuda") for _ in imgs]
    t = CS.to_product(spec)
    return lambda: V.remap_tensors(t, srcs, dsts, radius=radius, interpolation=interp, boarder_value=bv, rotations=rots)


def calibration():
    cal = SO.calibration()
    print("calibration", {k: v for k, v in cal.items() if k not in ("a", "c")})
    for ms in (20.0, 100.0, 250.0):
        s = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        SO.stall(s, ms)
        e1.record(s)
        e1.synchronize()
        print(f"stall({ms}) measured {e0.elapsed_time(e1):.2f} ms")


def remap_family(S):
    _, spec, hw, out_wh, radius = PAIR_CASES[0]
    left, right = (SO.up(a) for a in frames(hw, 51))
    sbs = torch.empty((out_wh[1], 2 * out_wh[0], 3), dtype=torch.uint8, device="cuda")
    tp = CS.to_product(spec)
    timed(S, "apply_lr_tensors mirror pair", lambda: V.apply_lr_tensors(tp, left, right, out=sbs, size_output=out_wh, interpolation=1, radius=radius,
                                                                        boarder_value=(5, 6, 7)))
    timed(S, "remap_tensors mirror single", units(spec, frames(hw, 53)[:1], out_wh, radius, 1, (5, 6, 7)))
    spec0, (hs, ws), o0, r0, bv0 = C0
    timed(S, "remap_tensors tile K8 pair", units(spec0, [A.noise(np.uint8, hs, ws, 3, k) for k in range(2)], o0, r0, 4, bv0))
    timed(S, "remap_tensors cn BGRA pair", units(EQUI, [A.noise(np.uint8, 300, 320, 4, k) for k in range(2)], (613, 587), 140.0, 1, 77))
    (hs, ws), ob, sb, rb = LEAN_BATCH["m_table"]
    timed(S, "remap_tensors batch 11 units", units(sb, [A.noise(np.uint8, hs, ws, 3, k) for k in range(11)], ob, rb, 1, (5, 6, 7)))
    for n in (3, 17):
        imgs, specs = SO.rot_units(n, 600)
        timed(S, f"remap_tensors rot_pair {n} units", units(SO.ROT_BASE, imgs, (448, 448), 80.0, 1, (1, 2, 3), rots=[s[1][1] for s in specs]))
    g = WIDE_PLAIN
    timed(S, "remap_tensors wide float32", units(g["spec"], [A.noise(np.float32, *g["src_hw"], 3, 1)], g["out_wh"], g["radius"], 1, BV[np.float32],
                                                  dt=torch.float32))
    d2 = [SO.up(a) for a in SO.discs(300, 170, 158.5)]
    timed(S, "auto_radius_tensor of two images", lambda: R.auto_radius_tensor(d2))
    timed(S, "anaglyph_tensors", lambda: V.anaglyph_tensors(left, right))
    o288 = torch.empty((288, 576, 3), dtype=torch.uint8, device="cuda")
    ta = CS.to_product(SO.AUTO_SPEC)
    timed(S, "apply_lr_tensors radius=auto on device", lambda: V.apply_lr_tensors(ta, d2[0], d2[1], out=o288, size_output=(288, 288), interpolation=4,
                                                                                  boarder_value=(17, 200, 90), radius="auto", auto_radius_on_device=True))
    halves = [o288[:, :288], o288[:, 288:]]
    timed(S, "remap_tensors_auto", lambda: R.remap_tensors_auto(ta, d2, halves, interpolation=1, boarder_value=(17, 200, 90)))


def c_abi(S):
    lib = _native.lib()
    src, xm, ym, border, bv = noise_case(np.uint8, 3, 1)
    s_d, x_d, y_d = SO.up(src), SO.up(xm), SO.up(ym)
    out = torch.empty((200, 200, 3), dtype=torch.uint8, device="cuda")
    cv = R.border_scalar(bv)
    timed(S, "v1c_remap_lut", lambda: lib.v1c_remap_lut(0, S.cuda_stream, s_d.data_ptr(), 40, 60, 180, 3, out.data_ptr(), 200, 200, 600, x_d.data_ptr(),
                                                        y_d.data_ptr(), 800, 1, border, cv.ctypes.data))
    ch = lower_for_get_map(CS.to_product(PLAIN), radius=48.0, size_input=(96, 104), size_output=(88, 72))
    f_s, f_d = SO.up(A.noise(np.uint8, 96, 104, 3, 700)), torch.empty((72, 88, 3), dtype=torch.uint8, device="cuda")
    timed(S, "v1c_remap_fused", lambda: lib.v1c_remap_fused(0, S.cuda_stream, f_s.data_ptr(), 96, 104, 312, 3, f_d.data_ptr(), 72, 88, 264, C.byref(ch), 4,
                                                            0, cv.ctypes.data))
    ch2 = lower_for_get_map(CS.to_product(PLAIN), radius=96.0, size_input=(192, 208), size_output=(176, 144))
    plan = R._plan_for(ch2, src_hw=(192, 208), dst_wh=(176, 144), cn=3, interpolation=1, border_mode=0, border_value=0, device=torch.device("cuda", 0))
    timed(S, "Plan.get_map (v1c_plan_get_map)", lambda: plan.get_map())


def circle_and_features(S):
    img = SO.up(CC.shared_cases()["aa_disc_1"].img)
    timed(S, "fit_circle_tensor (v1c_fit_circle_async)", lambda: circle.fit_circle_tensor(img))
    a, b = feature_pair()
    p = F.params(1.0, 48.0)
    ta, tb = SO.up(a), SO.up(b)
    timed(S, "v1c_feat_detect", lambda: F._detect_enqueue(ta, p))
    _, da, ca = F._detect_enqueue(ta, p)
    _, db, cb = F._detect_enqueue(tb, p)
    na, nb = int(ca.cpu()[0]), int(cb.cpu()[0])
    timed(S, "v1c_feat_match", lambda: F._match_enqueue(da[:na], db[:nb], p))


def main():
    _native.lib()
    calibration()
    S = torch.cuda.Stream()
    remap_family(S)
    c_abi(S)
    circle_and_features(S)
    worst = max(ROWS, key=lambda r: r[1])
    print(f"slowest (median): {worst[0]} {worst[1]:.3f} ms; slowest single call: {max(r[2] for r in ROWS):.3f} ms")


if __name__ == "__main__":
    main()
