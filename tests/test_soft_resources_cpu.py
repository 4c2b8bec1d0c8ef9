"""Static resource checks of the SOFTENED walk kernels (no GPU needed: hipcc cross-compiles) -- the limits of
tests/test_kernel_resources_cpu.py applied to walk_fast_soft_kernel and walk_f64_soft_kernel.

A softened kernel is its unsoftened twin plus one add per reciprocal square root, with eps2 held in a VGPR (fp32) or a VGPR
pair (fp64).  It must keep the twin's resident-wave count: no scratch, no spills, the same SGPR ceilings (<= 80 for the
one-wave-per-group fp32 loop and for every fp64 assembly kernel: 8 resident waves per SIMD), <= 64 VGPRs.  And the add must
be there, once per v_rsq, inside the hand-written loops."""
import re

import pytest

import kernel_meta as KM

SOFT = re.compile(r"_ZN2bh21walk_fast_soft_kernelILb([01])ELb([01])ELi(\d+)ELb([01])EEEvNS_12WalkFastArgsE")   # <LDS_STACK, STATS, SPLIT, ASM>
PLAIN = "_ZN2bh16walk_fast_kernel"
F64_SOFT = re.compile(r"_ZN2bh20walk_f64_soft_kernelILb([01])ELb([01])ELb([01])ELb([01])EEEv")    # <COMPAT, STATS, DEEP, ASM>


@pytest.fixture(scope="module")
def fast_asm():
    return KM.assembly("bh_walk_fast.hip", diagnostics=True)[0]


@pytest.fixture(scope="module")
def engine_asm():
    return KM.assembly("bh_engine.hip")[0]


def _body(text, name):
    """The code of kernel `name`: from its label to the end of the function."""
    body = text[text.index("\n" + name + ":"):]
    return body[:body.index(".Lfunc_end")]


def test_every_softened_fp32_walk_kernel_keeps_its_twins_limits(fast_asm):
    ks = KM.kernels(fast_asm, r"_ZN2bh21walk_fast_soft_kernel\S+")
    plain = KM.kernels(fast_asm, PLAIN + r"\S+")
    assert len(ks) == len(plain) == 14                        # every instantiation the launcher reaches has a softened twin
    asm = {k: v for k, v in ks.items() if SOFT.match(k).group(4) == "1"}
    assert sorted(int(SOFT.match(k).group(3)) for k in asm) == [1, 2, 4, 8]
    for name, r in asm.items():
        split = int(SOFT.match(name).group(3))
        assert r["scratch"] == 0 and r["dynamic_stack"] == "false", (name, r)
        assert r["sgpr_spill"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["vgpr"] <= 64, (name, r)
        assert r["sgpr"] <= (80 if split == 1 else 106), (name, r)
    for name, r in ks.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        twin = plain[name.replace("_ZN2bh21walk_fast_soft_kernel", PLAIN)]
        # the same SGPR allocation granule (count + 16 rounded up to 16) and at most 64 VGPRs: the twin's resident waves
        assert (r["sgpr"] + 16 + 15) // 16 == (twin["sgpr"] + 16 + 15) // 16, (name, r, twin)
        assert r["vgpr"] <= 64, (name, r)


def test_the_softened_fp32_loops_add_eps2_once_per_rsq_and_the_plain_ones_never(fast_asm):
    ks = KM.kernels(fast_asm, r"_ZN2bh21walk_fast_soft_kernel\S+")
    assert len(ks) == 14                                      # (nothing to iterate over would pass everything below)
    for name in ks:
        body = _body(fast_asm, name)
        twin = _body(fast_asm, name.replace("_ZN2bh21walk_fast_soft_kernel", PLAIN))
        n_rsq = body.count("v_rsq_f32")
        assert n_rsq == twin.count("v_rsq_f32") > 0, name
        assert body.count("v_add_f32") - twin.count("v_add_f32") == n_rsq, name
        if SOFT.match(name).group(4) == "1":                  # the hand-written blocks: in place on d2, right before the rsq
            assert len(re.findall(r"v_add_f32_e32 v24, v\d+, v24\n\s*v_rsq_f32_e32 v25, v24", body)) >= 9, name     # (eight child blocks and the bucket loop at the least)
            assert "v_add_f32_e32 v24" not in twin


def test_every_softened_fp64_walk_kernel_keeps_its_twins_limits(engine_asm):
    ks = KM.kernels(engine_asm, r"_ZN2bh20walk_f64_soft_kernel\S+")
    plain = KM.kernels(engine_asm, r"_ZN2bh15walk_f64_kernel\S+")
    assert len(ks) == len(plain) == 12
    asm = {k: v for k, v in ks.items() if F64_SOFT.match(k).group(4) == "1"}
    assert sorted((F64_SOFT.match(k).group(1), F64_SOFT.match(k).group(3)) for k in asm) == [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")]
    for name, r in asm.items():
        assert F64_SOFT.match(name).group(2) == "0", name
        assert r["scratch"] == 0 and r["dynamic_stack"] == "false", (name, r)
        assert r["sgpr_spill"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["sgpr"] <= 80 and r["vgpr"] <= 64, (name, r)
        body = _body(engine_asm, name)
        assert "s_load_dwordx16 s[24:39]" in body and "s_load_dwordx16 s[40:55]" in body and "s_load_dwordx8 s[56:63]" in body
        assert body.count("v_cmpx_lt_f64_e32") == 4
        # one add per child of the hand-written loop, in place on d2 and right in front of its v_rsq_f64
        assert len(re.findall(r"v_add_f64 v\[28:29\], v\[28:29\], v\[\d+:\d+\]\n\s*v_rsq_f64_e32 v\[30:31\], v\[28:29\]", body)) == 4, name
        twin = _body(engine_asm, name.replace("_ZN2bh20walk_f64_soft_kernel", "_ZN2bh15walk_f64_kernel"))
        assert "v_add_f64 v[28:29], v[28:29]" not in twin
    for name, r in ks.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
        twin = plain[name.replace("_ZN2bh20walk_f64_soft_kernel", "_ZN2bh15walk_f64_kernel")]
        assert (r["sgpr"] + 16 + 15) // 16 == (twin["sgpr"] + 16 + 15) // 16 and r["vgpr"] <= 64, (name, r, twin)
