"""Register and scratch budget of the image-circle kernels (csrc/kernels_circle.hip), read from the code object's metadata notes the
way tests/test_resource_budget.py reads the remap kernels': no kernel uses scratch or spills a register, and the fit's one workgroup of
512 threads -- two waves per SIMD -- fits the register file (at most 256 VGPRs per lane)."""
from pathlib import Path

import pytest

from test_resource_budget import CSRC, kernel_metadata


@pytest.fixture(scope="module")
def circle_kernels(tmp_path_factory, product_lib):
    obj = CSRC / "kernels_circle.o"
    assert obj.exists(), "kernels_circle.o is built by __graft_entry__.build() / make"
    return kernel_metadata(tmp_path_factory.mktemp("meta_circle"), Path(obj))


def test_circle_kernels_use_no_scratch_and_spill_nothing(circle_kernels):
    names = [k[".name"] for k in circle_kernels]
    # rows and column bands for uint8 / uint16 x 1 / 3 / 4 channels, the column join and the fit
    assert len(names) == 14 and sum("k_circle_rows" in n for n in names) == 6 and sum("k_circle_col_bands" in n for n in names) == 6
    bad = [(k[".name"], k[".private_segment_fixed_size"], k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for k in circle_kernels
           if k[".private_segment_fixed_size"] or k[".sgpr_spill_count"] or k[".vgpr_spill_count"]]
    assert not bad, bad


def test_fit_workgroup_fits_the_register_file(circle_kernels):
    fit = [k for k in circle_kernels if "k_circle_fit" in k[".name"]]
    assert len(fit) == 1
    assert fit[0][".max_flat_workgroup_size"] == 512 and fit[0][".vgpr_count"] <= 256, fit[0]
    assert fit[0][".group_segment_fixed_size"] <= 8 * 10 * 8 + 4 * 8 + 32768 * 4  # sums, broadcast and the cached points: under 160 KiB
