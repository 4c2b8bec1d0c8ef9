"""Static resource checks of the radial kernels of csrc/bh_radial.hpp (no GPU needed: hipcc cross-compiles): every
instantiation of radial_max_kernel, radial_deposit_kernel and radial_select_kernel runs without scratch memory and without
register spills, and the LDS the two histogram kernels declare statically stays inside the 64 KiB a launch may ask for."""
import re

import pytest

import kernel_meta as KM

KERNELS = {"radial_max_kernel": 4,"radial_deposit_kernel": 4, "radial_select_kernel": 2}     # name -> instantiations


@pytest.fixture(scope="module")
def engine_asm():
    return KM.assembly("bh_engine.hip")[0]


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_scratch_and_no_spills(engine_asm, kernel):
    ks = KM.kernels(engine_asm, r"_ZN2bh\d+" + kernel + r"\S+")
    assert len(ks) == KERNELS[kernel], sorted(ks)
    for name, r in ks.items():
        assert r["scratch"] == 0 and r["dynamic_stack"] == "false", (name, r)
        assert r["sgpr_spill"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)                     # at least four waves per SIMD


def test_static_lds_fits_a_launch(engine_asm):
    for kernel, most in (("radial_select_kernel", 32 * 1024), ("radial_deposit_kernel", 64), ("radial_max_kernel", 12 * 1024)):
        found = 0
        for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n){0,12}?\s+\.name:\s+_ZN2bh\d+" + kernel, engine_asm):
            found += 1
            assert int(m.group(1)) <= most, (kernel, m.group(1))
        assert found == KERNELS[kernel], (kernel, found)
