"""Static resource checks of the azimuthal-mode kernels of csrc/bh_modes.hpp (no GPU needed: hipcc cross-compiles): every
instantiation of modes_max_kernel and modes_deposit_kernel -- {rates, no rates} x {fp32, fp64 state} -- runs without scratch
memory, without register spills and without a dynamic stack; the deposit declares no static LDS at all (its private histogram
may take the whole 64 KiB of dynamic LDS a launch can ask for), the first pass 2 x 256 doubles and 256 flags; and the run-time
harmonic loop keeps the registers of the deposit where a workgroup of 256 threads can share a SIMD with others."""
import re

import pytest

import kernel_meta as KM

KERNELS = {"modes_max_kernel": 4, "modes_deposit_kernel": 4}                   # name -> instantiations
STATIC_LDS = {"modes_max_kernel": 2 * 256 * 8 + 256 * 4, "modes_deposit_kernel": 0}
# recorded at this commit (hipcc -O3, gfx950), {no rates, rates} x {fp64, fp32 state}: modes_max_kernel 34 / 32 / 38 / 38 VGPRs and
# 44 / 44 / 54 / 56 SGPRs; modes_deposit_kernel 31 / 31 / 33 / 33 VGPRs and 63 / 63 / 84 / 84 SGPRs (the radial deposit: 34 - 38 and
# 58 - 67).  The bounds: 64 VGPRs keep eight waves on a SIMD; 102 SGPRs is all a wave has.
VGPR_MOST = {"modes_max_kernel": 64, "modes_deposit_kernel": 64}
SGPR_MOST = {"modes_max_kernel": 102, "modes_deposit_kernel": 102}


@pytest.fixture(scope="module")
def engine_asm():
    return KM.assembly("bh_engine.hip")[0]


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_scratch_and_no_spills(engine_asm, kernel):
    ks = KM.kernels(engine_asm, r"_ZN2bh\d+" + kernel + r"\S+")
    assert len(ks) == KERNELS[kernel], sorted(ks)
    for name, r in ks.items():
        print(name, r)
        assert r["scratch"] == 0 and r["dynamic_stack"] == "false", (name, r)
        assert r["sgpr_spill"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["vgpr"] <= VGPR_MOST[kernel] and r["sgpr"] <= SGPR_MOST[kernel], (name, r)


def test_static_lds_is_as_designed(engine_asm):
    for kernel, want in STATIC_LDS.items():
        found = 0
        for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n){0,12}?\s+\.name:\s+_ZN2bh\d+" + kernel, engine_asm):
            found += 1
            assert int(m.group(1)) == want, (kernel, m.group(1))
        assert found == KERNELS[kernel], (kernel, found)


def test_the_fast_walk_unit_does_not_see_the_header():
    import os
    src = open(os.path.join(KM.CSRC, "bh_walk_fast.hip")).read()
    assert "bh_modes.hpp" not in src and "bh_radial.hpp" not in src
    assert "bh_modes.hpp" in open(os.path.join(KM.CSRC, "bh_engine.hip")).read()
