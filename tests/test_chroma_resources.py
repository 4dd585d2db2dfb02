"""Register, scratch and LDS budget of the chromatic-aberration kernels (csrc/kernels_chroma.hip), read from the code object's metadata
notes the way tests/test_resource_budget.py reads the remap kernels': no ray-mode instantiation uses scratch or spills a register; the
literal and fix-up instantiations and the map kernels keep the interpreter's op loop and libm calls -- a slow path by construction, with
the allowance tests/test_resource_budget.py gives k_remap / k_get_map --; no kernel uses LDS."""
import re
from pathlib import Path

import pytest

from test_resource_budget import CSRC, kernel_metadata

MODE_LITERAL, MODE_RAY, MODE_FIXUP = 0, 1, 3  # csrc/kernels.hpp
INTERPS = (0, 1, 2, 4)                        # NEAREST, LINEAR, CUBIC, LANCZOS4


@pytest.fixture(scope="module")
def ca_kernels(tmp_path_factory, product_lib):
    obj = CSRC / "kernels_chroma.o"
    assert obj.exists(), "kernels_chroma.o is built by __graft_entry__.build() / make"
    return kernel_metadata(tmp_path_factory.mktemp("meta_chroma"), Path(obj))


def remap_instantiations(kernels):
    """{(interp, mode): metadata} of k_remap_ca<INTERP, MODE>"""
    out = {}
    for k in kernels:
        m = re.search(r"k_remap_caILi(\d+)ELi(\d+)E", k[".name"])
        if m:
            out[(int(m.group(1)), int(m.group(2)))] = k
    return out


def test_the_instantiations_are_the_designs(ca_kernels):
    inst = remap_instantiations(ca_kernels)
    assert sorted(inst) == sorted((i, m) for i in INTERPS for m in (MODE_LITERAL, MODE_RAY, MODE_FIXUP))
    assert sum("k_get_map_ca" in k[".name"] for k in ca_kernels) == 2 and len(ca_kernels) == 14
    for k in ca_kernels:
        assert k[".max_flat_workgroup_size"] == 256, k[".name"]
        # the one by-value argument block sits at byte 0 of the kernel-argument segment: the kernels read it from there
        assert k[".args"][0][".offset"] == 0 and k[".args"][0][".value_kind"] == "by_value", k[".name"]


def test_ray_mode_uses_no_scratch_and_spills_nothing(ca_kernels):
    inst = remap_instantiations(ca_kernels)
    bad = [(i, k[".private_segment_fixed_size"], k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for (i, m), k in inst.items()
           if m == MODE_RAY and (k[".private_segment_fixed_size"] or k[".sgpr_spill_count"] or k[".vgpr_spill_count"])]
    assert not bad, bad
    # NEAREST / LINEAR / CUBIC hold six waves per SIMD (512 VGPRs / 6 = 85; 76 at the time of writing), LANCZOS4
    # three (512 / 3 = 170; 167)
    for i in (0, 1, 2):
        assert inst[(i, MODE_RAY)][".vgpr_count"] <= 84, (i, inst[(i, MODE_RAY)][".vgpr_count"])
    assert inst[(4, MODE_RAY)][".vgpr_count"] <= 168, inst[(4, MODE_RAY)][".vgpr_count"]


def test_no_kernel_spills_vector_registers_and_the_design_has_no_lds(ca_kernels):
    """The kernels declare no LDS.  In the Lanczos4 instantiations the compiler keeps the border path's eight column indices per lane in
    LDS instead of registers (256 lanes x 8 x 4 B = 8 KiB per workgroup, a twentieth of a CU's 160 KiB: no bound on occupancy); every
    other instantiation has none."""
    inst = remap_instantiations(ca_kernels)
    for k in ca_kernels:
        assert k[".vgpr_spill_count"] == 0, k[".name"]
    for (i, m), k in inst.items():
        lds = k[".group_segment_fixed_size"]
        assert lds in (0, 256 * 8 * 4) if i == 4 else lds == 0, (k[".name"], lds)
