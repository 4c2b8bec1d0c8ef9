"""CPU checks of the diagnostics interface (bh_compute_potential, bh_get_potential, bh_energy) and of the tests'
own reference potential (tests/potential_ref.py)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

from oracle import bh_oracle as O
from gpu_nbody_simulation_amd import _lib
from gpu_nbody_simulation_amd.engine import BhEnergy
from potential_ref import potential_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bhgpu.h")
NEW = ("bh_compute_potential", "bh_get_potential", "bh_energy")


def test_the_diagnostics_are_declared_exported_and_bound():
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()
    for name in NEW:
        assert getattr(lib, name) is not None
    assert _lib.ABI_VERSION == 4 and lib.bh_abi_version() == 4          # added functions only
    assert [f.name for f in __import__("dataclasses").fields(BhEnergy)][:3] == ["kinetic", "potential", "total"]


def test_energy_struct_layout_matches_the_header(tmp_path):
    fields = [f[0] for f in _lib.bh_energy_t._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("%zu\\n", sizeof(bh_energy_t));']
    lines += [f'printf("%zu\\n", offsetof(bh_energy_t, {f}));' for f in fields]
    lines.append("return 0;}")
    prog = tmp_path / "energy_layout.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "energy_layout"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(prog)])
    out = list(map(int, subprocess.check_output([str(exe)]).decode().split()))
    assert out[0] == C.sizeof(_lib.bh_energy_t) == 80
    assert out[1:] == [getattr(_lib.bh_energy_t, f).offset for f in fields]


def test_reference_walk_equals_the_direct_sum_when_every_cell_is_opened():
    """theta -> 0 on the uncapped tree (max_depth 32): every body meets every other as a single-body leaf."""
    rng = np.random.default_rng(7)
    n = 600
    p = rng.uniform(-1.0, 1.0, (n, 2))
    m = rng.uniform(0.1, 0.5, n)
    G = 1.0
    phi, cnt = potential_walk(O.build_tree(p, m, 0), p, theta=1e-9, G=G, compat=False)
    assert np.array_equal(cnt, np.full(n, n - 1))
    for i in range(0, n, 37):
        d = np.sqrt(((p - p[i]) ** 2).sum(axis=1)) + 1e-15
        ref = -G * math.fsum(np.delete(m / d, i))
        assert abs(phi[i] - ref) <= 1e-13 * abs(ref)


def test_reference_walk_counts_equal_the_oracle_counts():
    """The reference walk takes the oracle force walk's nodes: its per-body counts are compute_forces_diag's."""
    rng = np.random.default_rng(3)
    p = rng.normal(0.0, 1.0, (3000, 2))
    m = rng.uniform(0.1, 0.5, 3000)
    for md, compat in ((10, True), (32, False)):
        nodes = O.build_tree(p, m, md if md < 32 else 0)
        _, cnt = potential_walk(nodes, p, theta=0.5, compat=compat)
        d = O.compute_forces_diag(nodes, p, m, theta=0.5, compat_self_skip=compat)
        assert np.array_equal(cnt, d.counts.astype(np.int64))
