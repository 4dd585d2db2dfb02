"""Register, scratch and LDS budget of the vignetting kernels (csrc/kernels_vignette.hip), read from the code object's metadata notes
the way tests/test_colormatch_resources.py reads the colour match's: no kernel uses scratch or spills a register, and every kernel's
LDS is the figure its design gives."""
from pathlib import Path

import pytest

from test_resource_budget import CSRC, kernel_metadata

TABLES = 3 * 1025 * 2  # three tables of 1025 uint16 in Q14


@pytest.fixture(scope="module")
def vig_kernels(tmp_path_factory, product_lib):
    obj = CSRC / "kernels_vignette.o"
    assert obj.exists(), "kernels_vignette.o is built by __graft_entry__.build() / make"
    return kernel_metadata(tmp_path_factory.mktemp("meta_vignette"), Path(obj))


def test_vignette_kernels_use_no_scratch_and_spill_nothing(vig_kernels):
    names = [k[".name"] for k in vig_kernels]
    # the gain pass and the ring statistics for uint8 / uint16 x 1 / 3 / 4 channels, and the launch that zeroes the record
    assert len(names) == 13 and sum("k_vig_zero" in n for n in names) == 1
    assert sum("k_vig_apply" in n for n in names) == 6 and sum("k_vig_rings" in n for n in names) == 6
    bad = [(k[".name"], k[".private_segment_fixed_size"], k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for k in vig_kernels
           if k[".private_segment_fixed_size"] or k[".sgpr_spill_count"] or k[".vgpr_spill_count"]]
    assert not bad, bad


def test_lds_sizes_and_registers_are_the_designs(vig_kernels):
    for k in vig_kernels:
        lds, name = k[".group_segment_fixed_size"], k[".name"]
        if "k_vig_apply" in name:
            assert lds == TABLES == 6150, (name, lds)
            assert k[".max_flat_workgroup_size"] == 256
            # four workgroups of four waves per CU -- what the launch's 1024 workgroups count on -- fit while a wave keeps to 128 VGPRs
            assert k[".vgpr_count"] <= 128, (name, k[".vgpr_count"])
        elif "k_vig_rings" in name:
            # the per-wave copies are sized by the launch: 4 waves x rings x 4 words x 4 B, 1 KiB (16 rings) to 64 KiB (1024)
            assert lds == 0 and k[".uses_dynamic_stack"] is False, (name, lds)
            assert k[".max_flat_workgroup_size"] == 256 and k[".vgpr_count"] <= 128, (name, k[".vgpr_count"])
        else:
            assert lds == 0, (name, lds)
