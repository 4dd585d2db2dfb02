"""Register, scratch and LDS budget of the colour-match kernels (csrc/kernels_colormatch.hip), read from the code object's metadata notes
the way tests/test_resource_budget.py reads the remap kernels': no kernel uses scratch or spills a register, and every kernel's LDS is
the figure its design gives."""
from pathlib import Path

import pytest

from test_resource_budget import CSRC, kernel_metadata

COPY = 2 * 3 * 256 * 4  # one wave's histograms: 2 eyes x 3 channels x 256 bins x 4 B = 6 KiB
WAVES = 4               # of a workgroup of 256 threads


@pytest.fixture(scope="module")
def cm_kernels(tmp_path_factory, product_lib):
    obj = CSRC / "kernels_colormatch.o"
    assert obj.exists(), "kernels_colormatch.o is built by __graft_entry__.build() / make"
    return kernel_metadata(tmp_path_factory.mktemp("meta_colormatch"), Path(obj))


def test_colormatch_kernels_use_no_scratch_and_spill_nothing(cm_kernels):
    names = [k[".name"] for k in cm_kernels]
    # the histogram and the apply pass for 1 / 3 / 4 channels, the tables, and the launch that zeroes the workspace
    assert len(names) == 8 and sum("k_cm_zero" in n for n in names) == 1 and sum("k_cm_hist" in n for n in names) == 3 and sum("k_cm_apply" in n for n in names) == 3
    assert sum("k_cm_luts" in n for n in names) == 1
    bad = [(k[".name"], k[".private_segment_fixed_size"], k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for k in cm_kernels
           if k[".private_segment_fixed_size"] or k[".sgpr_spill_count"] or k[".vgpr_spill_count"]]
    assert not bad, bad


def test_lds_sizes_are_the_designs(cm_kernels):
    for k in cm_kernels:
        lds, name = k[".group_segment_fixed_size"], k[".name"]
        if "k_cm_hist" in name:
            assert lds == WAVES * COPY == 24576, (name, lds)  # a copy per wave
            assert k[".max_flat_workgroup_size"] == 64 * WAVES
        elif "k_cm_zero" in name:
            assert lds == 0, (name, lds)
        elif "k_cm_apply" in name:
            assert lds == 3 * 256, (name, lds)  # the tables
        else:
            # the counts of both eyes, scanned in place (one copy), the populated-bin masks of 2 x 3 histograms and the knot masks of 3
            # (four 64-bit words each), and four per-wave partial sums of 2 x 3 int64 sums
            assert lds == COPY + (6 + 3) * 4 * 8 + 6 * 4 * 8 == 6624, (name, lds)
            assert k[".max_flat_workgroup_size"] == 256
