"""Static resource checks of the disc kernels of csrc/bh_disc.hpp (no GPU needed: hipcc cross-compiles): every instantiation
of disc_init_kernel (fp32 and fp64 state), curve_max_kernel and curve_deposit_kernel (fp32, mixed, fp64 tree) and
disc_velocities_kernel (fp32 and fp64 state) runs without scratch memory, without register spills and without a dynamic stack,
in at most 64 VGPRs (eight waves on a SIMD); the deposit and the velocities declare no static LDS (a private histogram and the
tables are dynamic), the first pass 4 x 256 doubles and 256 flags."""
import os
import re

import pytest

import kernel_meta as KM

KERNELS = {"disc_init_kernel": 2, "curve_max_kernel": 3, "curve_deposit_kernel": 3, "disc_velocities_kernel": 2}
STATIC_LDS = {"disc_init_kernel": 0, "curve_max_kernel": 4 * 256 * 8 + 256 * 4, "curve_deposit_kernel": 0, "disc_velocities_kernel": 0}
VGPR_MOST, SGPR_MOST = 64, 102


@pytest.fixture(scope="module")
def engine_asm():
    return KM.assembly("bh_engine.hip")[0]


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_scratch_no_spills_and_at_most_64_vgprs(engine_asm, kernel):
    ks = KM.kernels(engine_asm, r"_ZN2bh\d+" + kernel + r"\S+")
    assert len(ks) == KERNELS[kernel], sorted(ks)
    for name, r in ks.items():
        print(name, r)
        assert r["scratch"] == 0 and r["dynamic_stack"] == "false", (name, r)
        assert r["sgpr_spill"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["vgpr"] <= VGPR_MOST and r["sgpr"] <= SGPR_MOST, (name, r)


def test_static_lds_is_as_designed(engine_asm):
    for kernel, want in STATIC_LDS.items():
        found = 0
        for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n){0,12}?\s+\.name:\s+_ZN2bh\d+" + kernel, engine_asm):
            found += 1
            assert int(m.group(1)) == want, (kernel, m.group(1))
        assert found == KERNELS[kernel], (kernel, found)


def included_from(unit):
    """Every file of csrc/ that `unit` includes with quotes, directly or through another."""
    seen, todo = set(), [unit]
    while todo:
        name = todo.pop()
        if name in seen or not os.path.exists(os.path.join(KM.CSRC, name)):
            continue
        seen.add(name)
        todo += re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(KM.CSRC, name)).read(), flags=re.M)
    return seen


def test_the_fast_walk_unit_does_not_see_the_header():
    fast, engine = included_from("bh_walk_fast.hip"), included_from("bh_engine.hip")
    assert "bh_walk_fast_body.hpp" in fast and "bh_prims.hpp" in fast, sorted(fast)      # (the walk is followed through its headers)
    assert "bh_disc.hpp" not in fast and "bh_disc.hpp" in engine
    # the pieces the header reuses are not copied into it
    disc = open(os.path.join(KM.CSRC, "bh_disc.hpp")).read()
    for reused in ("struct Philox", "double u01(", "int radial_slot(", "bool map_finite(", "struct RadCentre", "kRadMinR2 ="):
        assert reused not in disc, reused
