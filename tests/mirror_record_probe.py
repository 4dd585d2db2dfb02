"""Helper of test_gpu_mirror_record.py::test_tuning_twin_keeps_the_box_prologue: pairs and one image through the mirror launch of
whatever library V1C_LIB names, compared with the oracle; run in a subprocess because the engine reads V1C_MIRROR_REC once per
process.  Prints 'OK' on success."""
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
for spec, hw, out, radius in ((equi, (300, 300), (448, 448), 150.0), (poly, (120, 120), (1024, 1024), 60.0)):  # rest tiles / none
    l, r = noise_disc(*hw, 81), noise_disc(*hw, 82)
    got = V.apply_lr_tensors(CS.to_product(spec), torch.from_numpy(l).to(dev), torch.from_numpy(r).to(dev), size_output=out,
                             interpolation=1, radius=radius).cpu().numpy()
    assert remapper.last_launch_kinds() == ["mirror"], remapper.last_launch_kinds()
    assert np.array_equal(got, O.apply_lr(spec, l, r, size_output=out, interpolation=1, radius=radius)), ("pair", hw)
    dst = torch.empty((out[1], out[0], 3), dtype=torch.uint8, device=dev)
    V.remap_tensors(CS.to_product(spec), [torch.from_numpy(l).to(dev)], [dst], radius=radius, interpolation=1)
    assert remapper.last_launch_kinds() == ["mirror"], remapper.last_launch_kinds()
    assert np.array_equal(dst.cpu().numpy(), O.apply(spec, [l], size_output=out, interpolation=1, radius=radius)[0]), ("one", hw)
print("OK")
