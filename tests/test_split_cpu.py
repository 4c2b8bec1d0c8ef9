"""The split operators without a GPU: the twin tests/split_ref.py against integrator_ref.kick_drift, the teeth of the
fixture tests/test_gpu_split.py runs on the device, the C declarations and ctypes signatures of the four entry points, and
static checks of the new kernels' code (hipcc cross-compiles).

The instruction checks ask for FUSED arithmetic where csrc/bh_split.hpp writes fma(), and for a separate product and sum in
the F64_EXACT kernels.  The compiler encodes a fused multiply-add of this shape as v_pk_fma_f32 (both components of a float2
in one instruction) and as v_fmac_f64 (the accumulate form, destination = addend); both are the single-rounding
v_fma_f32 / v_fma_f64 operation, so the checks accept the family and refuse any v_mul / v_add pair in its place.  The fp64
division a = F / m_i expands into its own v_fma_f64 sequence that ends in v_div_fixup_f64: "the state update" is what
follows the last of those."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import integrator_ref as R
import kernel_meta as KM
import split_ref as S
from gpu_nbody_simulation_amd import _lib
from oracle import bh_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bhgpu.h")


# ---- the twin ----------------------------------------------------------------------------------------------------------
def _oracle_accel(m, p):
    t = O.build_tree(p, m, 0)
    return O.compute_forces(t, p, m, G=R.FIX_G, compat_self_skip=False) / m[:, None]


@pytest.fixture(scope="module")
def fixture1000():
    m, p, v = R.make_fixture(1000)
    return m, p, v, _oracle_accel(m, p)


@pytest.mark.parametrize("h", [R.FIX_DT, -R.FIX_DT / 2])
@pytest.mark.parametrize("kind", S.KINDS)
def test_drift_of_kick_is_the_fused_epilogue(fixture1000, kind, h):
    m, p, v, a = fixture1000
    if kind == "f32":
        p, v, a = R.to_f32(p), R.to_f32(v), R.to_f32(a)
    elif kind == "mixed":
        a = R.to_f32(a)
    vt, pt = R.kick_drift(a, v, p, h, kind)
    vn = S.kick(a, v, h, kind)
    pn = S.drift(vn, p, h, kind)
    assert np.array_equal(vn, vt) and np.array_equal(pn, pt)
    assert not np.array_equal(vn, v) and not np.array_equal(pn, p)


@pytest.mark.parametrize("kind", S.KINDS)
def test_h_zero_returns_the_state(fixture1000, kind):
    m, p, v, a = fixture1000
    if kind in ("f32", "mixed"):
        a = R.to_f32(a)
    if kind == "f32":
        p, v = R.to_f32(p), R.to_f32(v)
    assert np.array_equal(S.kick(a, v, 0.0, kind), v) and np.array_equal(S.drift(v, p, 0.0, kind), p)


def test_kinds_take_the_stated_types():
    a = np.array([[0.1, 0.2]])
    with pytest.raises(ValueError):
        S.kick(a, a, 0.01, "mixed")                           # 0.1 is no fp32 value
    with pytest.raises(ValueError):
        S.kick(a, a, 0.01, "leapfrog")
    with pytest.raises(ValueError):
        S.drift(a, a, 0.01, "leapfrog")


# ---- teeth -------------------------------------------------------------------------------------------------------------
def test_mixed_kick_with_rounded_h_is_told_apart(fixture1000):
    m, p, v, a = fixture1000
    a = R.to_f32(a)
    for h in (R.FIX_DT, R.FIX_DT / 2):
        assert float(np.float32(h)) != h
        frac = (S.kick(a, v, h, "mixed") != S.kick_mixed_rounded_h(a, v, h)).mean()
        print(f"mixed kick, h = {h}: h != f32(h) on {frac:.4f} of the velocity components")
        assert frac >= 0.3                                    # (a third of the fixture has exact-zero velocities: a * h alone, still told apart)


def test_unfused_fp32_kick_is_told_apart(fixture1000):
    m, p, v, a = (R.to_f32(x) for x in fixture1000)
    frac = (S.kick(a, v, R.FIX_DT, "f32") != S.kick_unfused32(a, v, R.FIX_DT)).mean()
    print(f"fp32 kick: fused != unfused on {frac:.4f} of the velocity components")
    assert frac >= 0.05


def test_exact_kind_is_unfused_and_f64_is_fused(fixture1000):
    m, p, v, a = fixture1000
    assert (S.kick(a, v, R.FIX_DT, "exact") != S.kick(a, v, R.FIX_DT, "f64")).mean() >= 0.05
    # (the drift on operands of the kick's proportions: on the fixture's own v dt is 1e-5 of p, and its rounding never shows)
    assert (S.drift(a, v, R.FIX_DT, "exact") != S.drift(a, v, R.FIX_DT, "f64")).mean() >= 0.05


def test_the_twin_reproduces_the_recorded_energy_errors():
    """the eccentric pair over t = 10, max |dE / E| sampled every step."""
    eu = [S.pair_energy_error(0.5, dt, 10.0, "euler") for dt in (0.02, 0.01, 0.005)]
    kd = [S.pair_energy_error(0.5, dt, 10.0, "kdk") for dt in (0.02, 0.01, 0.005)]
    assert np.allclose(eu, [7.59e-2, 3.71e-2, 1.83e-2], rtol=5e-3) and np.allclose(kd, [7.10e-3, 1.79e-3, 4.50e-4], rtol=5e-3)
    assert 1.8 <= eu[1] / eu[2] <= 2.3 and 3.5 <= kd[1] / kd[2] <= 4.5 and kd[1] < eu[1] / 10


# ---- declarations --------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_abi_stays_4():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(src.split())
    for decl in ("int bh_kick(bh_ctx *ctx, double h);", "int bh_drift(bh_ctx *ctx, double h);",
                 "int bh_timestep(bh_ctx *ctx, double eta, double length, bh_timestep_t *out);",
                 "int bh_step_kdk(bh_ctx *ctx, int32_t nsteps);"):
        assert decl in flat, decl
    assert re.search(r"#define BHGPU_ABI_VERSION 4\b", src)
    assert re.search(r"typedef struct bh_timestep_t \{ double dt; double a_max; int64_t worst; int64_t n_bodies; \} bh_timestep_t;", flat)


def test_ctypes_signatures():
    ctx, d = C.c_void_p, C.c_double
    assert _lib.SIGNATURES["bh_kick"] == (C.c_int, [ctx, d])
    assert _lib.SIGNATURES["bh_drift"] == (C.c_int, [ctx, d])
    assert _lib.SIGNATURES["bh_step_kdk"] == (C.c_int, [ctx, C.c_int32])
    res, args = _lib.SIGNATURES["bh_timestep"]
    assert res == C.c_int and args[:3] == [ctx, d, d] and args[3]._type_ is _lib.bh_timestep_t
    assert [(n, t) for n, t in _lib.bh_timestep_t._fields_] == [("dt", d), ("a_max", d), ("worst", C.c_int64), ("n_bodies", C.c_int64)]
    assert C.sizeof(_lib.bh_timestep_t) == 32 and _lib.ABI_VERSION == 4


def test_null_context_is_an_argument_error():
    lib = _lib.load()
    assert lib.bh_abi_version() == 4
    assert lib.bh_kick(None, 0.1) == -1 and lib.bh_drift(None, 0.1) == -1 and lib.bh_step_kdk(None, 1) == -1
    t = _lib.bh_timestep_t()
    assert lib.bh_timestep(None, 0.02, 1e-3, C.byref(t)) == -1


# ---- the kernels' code -----------------------------------------------------------------------------------------------------
NEW = r"_ZN2bh\d+(kick_f32|kick_mixed|kick_f64|kick_exact|drift_f32|drift_f64|drift_exact|timestep_partial|timestep_final)_kernel\S*"
FUSED32 = re.compile(r"\bv_(pk_)?fma(c)?_f32")
FUSED64 = re.compile(r"\bv_fma(c)?_f64")


@pytest.fixture(scope="module")
def engine_asm():
    return KM.assembly("bh_engine.hip")[0]


def _body(text, name):
    body = text[text.index("\n" + name + ":"):]
    return body[:body.index(".Lfunc_end")]


def _kernel(text, short):
    names = [k for k in KM.kernels(text, NEW) if re.match(r"_ZN2bh\d+" + short + r"_kernel", k)]
    assert len(names) == 1, (short, names)
    return _body(text, names[0])


def _update(body):
    """What follows the last division (or the whole kernel when it has none)."""
    return body[body.rindex("v_div_fixup_f64"):].split("\n", 1)[1] if "v_div_fixup_f64" in body else body


def test_every_new_kernel_is_there_without_scratch_or_spills(engine_asm):
    ks = KM.kernels(engine_asm, NEW)
    assert len(ks) == 10, sorted(ks)                          # seven operators, two instances of the first reduction pass, the second
    for name, r in ks.items():
        assert r["scratch"] == 0 and r["dynamic_stack"] == "false", (name, r)
        assert r["sgpr_spill"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["vgpr"] <= 64, (name, r)


@pytest.mark.parametrize("short", ["kick_f32", "drift_f32"])
def test_fp32_operators_are_fused(engine_asm, short):
    body = _kernel(engine_asm, short)
    assert FUSED32.search(body) and not re.search(r"\bv_(pk_)?(mul|add)_f32", body), short


@pytest.mark.parametrize("short", ["kick_mixed", "kick_f64", "drift_f64"])
def test_fp64_operators_are_fused(engine_asm, short):
    upd = _update(_kernel(engine_asm, short))
    assert len(FUSED64.findall(upd)) == 2, short              # x and y
    assert not re.search(r"\bv_(mul|add)_f64", upd), short
    assert ("v_div_fixup_f64" in _kernel(engine_asm, short)) == (short == "kick_f64")     # a = F / m_i, IEEE


@pytest.mark.parametrize("short", ["kick_exact", "drift_exact"])
def test_exact_operators_keep_product_and_sum_apart(engine_asm, short):
    body = _kernel(engine_asm, short)
    upd = _update(body)
    assert len(re.findall(r"\bv_mul_f64", upd)) == 2 and len(re.findall(r"\bv_add_f64", upd)) == 2, short
    assert not FUSED64.search(upd), short
    assert (body.count("v_div_fixup_f64") == 2) == (short == "kick_exact")
    if short == "drift_exact":
        assert not FUSED64.search(body)
