"""Helper of test_gpu_tap_table_compact.py::test_tuning_twin_runs_both_table_chains_in_the_compact_form: the two rest-free chains of
tests/test_gpu_tap_table.py (the w-table POLY chain, the m-table EQUI chain) through the mirror launch of whatever library V1C_LIB names,
compared with the oracle; run in a subprocess with V1C_TAP_FORM=8 because the engine reads the switch from the environment of its
process.  The plans must then hold 8-byte entries although their tables are far below the size at which the product chooses them.
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
for spec, hw, out, radius, want_bytes in ((poly, (1024, 1024), (1024, 1024), 512.0, 16 * 33 * 2048), (equi, (300, 300), (448, 448), 146.0, 7 * 15 * 2048)):
    l, r = noise_disc(*hw, 81), noise_disc(*hw, 82)
    want = O.apply_lr(spec, l, r, size_output=out, interpolation=1, radius=radius)
    for _ in range(2):  # (the second call reuses the plan)
        got = V.apply_lr_tensors(CS.to_product(spec), torch.from_numpy(l).to(dev), torch.from_numpy(r).to(dev), size_output=out,
                                 interpolation=1, radius=radius).cpu().numpy()
        assert remapper.last_launch_kinds() == ["mirror"], remapper.last_launch_kinds()
        assert remapper.last_tap_table_bytes() == [want_bytes], remapper.last_tap_table_bytes()
        assert remapper.last_tap_entry_bytes() == [8], remapper.last_tap_entry_bytes()
        assert np.array_equal(got, want), ("pair", hw, int((got != want).sum()))
print("OK")
