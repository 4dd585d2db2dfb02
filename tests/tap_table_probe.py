"""Helper of test_gpu_tap_table.py::test_tuning_twin_has_the_computing_kernel_as_ab_partner: rest-free pairs of both table chains
through the mirror launch of whatever library V1C_LIB names, compared with the oracle; run in a subprocess because the engine reads
V1C_MIRROR_TAB once per process.  The plans hold their tables either way (the switch selects the kernel, not the plan's content).
Prints 'OK' on success."""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import chainspecs as CS  # noqa: E402
import vr180_convert_amd as V  # noqa: E402
from oracle import oracle as O  # noqa: E402
from vr180_convert_amd import remapper  # noqa: E402
from vr180_convert_amd.synth import noise_disc  # noqa: E402

O.build()
dev = torch.device("cuda", 0)
equi = [("equirect_enc", True), CS.EQUI]
poly = [("equirect_enc", True), ("poly", [0, 1, -0.1]), CS.EQUI]
for spec, hw, out, radius in ((equi, (300, 300), (448, 448), 146.0), (poly, (120, 120), (1024, 1024), 60.0)):
    l, r = noise_disc(*hw, 81), noise_disc(*hw, 82)
    for _ in range(2):  # (the second call reuses the plan)
        got = V.apply_lr_tensors(CS.to_product(spec), torch.from_numpy(l).to(dev), torch.from_numpy(r).to(dev), size_output=out,
                                 interpolation=1, radius=radius).cpu().numpy()
        assert remapper.last_launch_kinds() == ["mirror"], remapper.last_launch_kinds()
        assert remapper.last_tap_table_bytes() == [((out[0] + 63) // 64) * (out[1] // 32 + 1) * 3072], remapper.last_tap_table_bytes()
        assert np.array_equal(got, O.apply_lr(spec, l, r, size_output=out, interpolation=1, radius=radius)), ("pair", hw)
print("OK")
