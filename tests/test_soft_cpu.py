"""Plummer softening without a GPU: the softened numpy reference walks (tests/soft_ref.py) against their unsoftened
siblings and against the softened direct sum, the C-ABI additions, the command line, and LetStepper's agreement check."""
import ctypes as C
import os
import re
import socket

import numpy as np
import pytest

from oracle import bh_oracle as O
from gpu_nbody_simulation_amd import _lib
from gpu_nbody_simulation_amd import project
from direct_ref import direct_ref
from field_ref import field_walk, points_around
from forest_potential_ref import forest_potential
from potential_ref import potential_walk
import soft_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_eps_zero_is_the_unsoftened_helper_bit_for_bit(init1024):
    m, p, _ = init1024
    nodes = O.build_tree(p, m, 10)
    pts = points_around(p, 300, 3)
    for theta in (0.5, 0.2):
        a, b = field_walk(nodes, pts, theta=theta), SR.soft_field_walk(nodes, pts, theta=theta, eps=0.0)
        for f in ("accel", "phi", "abs_sum", "pot_sum", "margin"):
            assert np.array_equal(bits(getattr(a, f)), bits(getattr(b, f))), f
        assert np.array_equal(a.counts, b.counts)
        for compat in (True, False):
            ra, ca = potential_walk(nodes, p, theta=theta, compat=compat)
            rb, cb = SR.soft_potential_walk(nodes, p, theta=theta, compat=compat, eps=0.0)
            assert np.array_equal(bits(ra), bits(rb)) and np.array_equal(ca, cb)
    parts = [np.arange(r, len(m), 3) for r in range(3)]
    sample = np.arange(0, len(m), 7)
    fa, ca = forest_potential(m, p, parts, bodies=sample)
    fb, cb = SR.soft_forest_potential(m, p, parts, bodies=sample, eps=0.0)
    assert np.array_equal(bits(fa), bits(fb)) and np.array_equal(ca, cb)
    t = np.array([0, 1, 511, 1023])
    assert np.array_equal(bits(direct_ref(p, m, t)), bits(SR.soft_direct_ref(p, m, t, eps=0.0)))


@pytest.mark.parametrize("eps", [1e-2, 3e-2])
def test_leaves_only_walk_equals_the_softened_direct_sum(init1024, eps):
    """theta = 1e-9: every subdivided cell is opened, so a body's terms are the other bodies one by one (the tree is uncapped:
    one body per leaf), and the softened walk must be the softened direct sum up to summation order and the 1e-15 offset.
    The walk's distance carries the reference's + 1e-15 and the direct sum's does not: a term differs by up to 3e-15 / eps
    relative (d^-3), so the lengths here keep that below 3e-13 of a term (the box is 0.2 wide: both soften for real)."""
    m, p, _ = init1024
    n = len(m)
    nodes = O.build_tree(p, m, 0)
    r = SR.soft_field_walk(nodes, p, theta=1e-9, eps=eps, self_of=np.arange(n), compat=False)
    assert (r.counts == n - 1).all()
    ref = SR.soft_direct_ref(p, m, np.arange(n), eps=eps)
    f = r.accel * m[:, None]
    assert (np.linalg.norm(f - ref, axis=1) <= 1e-12 * np.linalg.norm(ref, axis=1)).all()
    # the potential of the same terms against the pair sum
    phi, cnt = SR.soft_potential_walk(nodes, p, theta=1e-9, compat=False, eps=eps)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
    t = m[None, :] / np.sqrt(d2 + eps * eps)
    np.fill_diagonal(t, 0.0)
    pair = -6.67e-11 * t.sum(axis=1)
    assert (cnt == n - 1).all() and (np.abs(phi - pair) <= 1e-12 * np.abs(pair)).all()
    assert (np.abs(r.phi - pair) <= 1e-12 * np.abs(pair)).all()
    # softening only shrinks: term by term, so sum by sum
    r0 = SR.soft_field_walk(nodes, p, theta=1e-9, eps=0.0, self_of=np.arange(n), compat=False)
    assert (r.abs_sum <= r0.abs_sum).all() and (r.pot_sum <= r0.pot_sum).all() and np.array_equal(r.counts, r0.counts)


def test_the_term_set_does_not_depend_on_eps(init1024):
    m, p, _ = init1024
    nodes = O.build_tree(p, m, 10)
    pts = points_around(p, 300, 3)
    base = SR.soft_field_walk(nodes, pts, eps=0.0)
    for eps in (1e-6, 1e-2, 10.0):
        r = SR.soft_field_walk(nodes, pts, eps=eps)
        assert np.array_equal(r.counts, base.counts) and np.array_equal(r.margin, base.margin)
        assert (r.abs_sum <= base.abs_sum).all()


def test_library_exports_the_softening_calls_and_the_abi_version_stays_4():
    hdr = open(os.path.join(ROOT, "include", "bhgpu.h")).read()
    assert re.search(r"int bh_set_softening\(bh_ctx \*ctx, double eps\);", hdr)
    assert re.search(r"int bh_get_softening\(bh_ctx \*ctx, double \*eps\);", hdr)
    assert re.search(r"#define BHGPU_ABI_VERSION 4\b", hdr)
    lib = C.CDLL(_lib.PRODUCT_LIB)
    for name in ("bh_set_softening", "bh_get_softening"):
        getattr(lib, name)                                   # AttributeError if not exported
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["bh_set_softening"] == (C.c_int, [C.c_void_p, C.c_double])
    assert _lib.ABI_VERSION == 4 and _lib.load().bh_abi_version() == 4
    # no struct changed: the binding's bh_config is the eleven fields it was
    assert [f[0] for f in _lib.bh_config._fields_][-1] == "node_capacity" and C.sizeof(_lib.bh_config) == 64
    # a null context is refused before anything is touched
    assert _lib.load().bh_set_softening(None, 0.1) == -1


def test_project_refuses_softening_in_the_bit_exact_precision(capsys):
    a, _ = project._parse(["--softening", "1e-3", "--precision", "f32"])
    assert a.softening == 1e-3
    a, _ = project._parse([])
    assert a.softening is None                                # without the flag nothing changes
    a, _ = project._parse(["--softening", "0"])               # 0 is the unsoftened law: accepted anywhere
    assert a.softening == 0.0
    for argv in (["--softening", "1e-3"], ["--softening", "1e-3", "--precision", "f64"]):
        with pytest.raises(SystemExit):
            project._parse(argv)
        assert "reference has no softening" in capsys.readouterr().err
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            project._parse(["--softening", bad, "--precision", "f32"])
        assert "finite and >= 0" in capsys.readouterr().err


# ---- LetStepper: eps is a property of the run ------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _let_worker(rank, world, port, eps_of_rank, out_dir):
    import torch
    import torch.distributed as dist
    from dist_standin import LetStandInEngine
    from gpu_nbody_simulation_amd.distributed import LetStepper

    class SoftStandIn(LetStandInEngine):
        seen = None

        def set_softening(self, eps):
            self.seen = eps

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rng = np.random.default_rng(rank)
        eng = SoftStandIn()
        eng.upload(rng.uniform(-1, 1, (16, 2)), np.zeros((16, 2)), np.ones(16))
        try:
            st = LetStepper(eng, rank, world, let_cap=64, device=torch.device("cpu"), softening=eps_of_rank[rank])
            res = "ok %r %r" % (st.softening, eng.seen)
        except ValueError as e:
            res = "ValueError %s" % e
        with open(os.path.join(out_dir, "r%d.txt" % rank), "w") as fh:
            fh.write(res)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("eps_of_rank,agree", [((0.25, 0.25), True), ((0.25, 0.125), False), ((0.0, 1e-3), False)])
def test_let_stepper_takes_eps_once_and_raises_when_the_ranks_disagree(tmp_path, eps_of_rank, agree):
    import torch.multiprocessing as mp
    mp.spawn(_let_worker, args=(2, _free_port(), eps_of_rank, str(tmp_path)), nprocs=2, join=True)
    for rank in range(2):
        res = open(tmp_path / ("r%d.txt" % rank)).read()
        if agree:
            assert res == "ok %r %r" % (eps_of_rank[rank], eps_of_rank[rank])
        else:
            assert res.startswith("ValueError") and "disagree on the softening length" in res


def test_let_stepper_defaults_to_no_softening_and_checks_its_argument():
    import torch
    from dist_standin import LetStandInEngine
    from gpu_nbody_simulation_amd.distributed import LetStepper
    eng = LetStandInEngine()                                  # (an engine without the setter: fine while eps is 0)
    eng.upload(np.zeros((4, 2)), np.zeros((4, 2)), np.ones(4))
    assert LetStepper(eng, 0, 1, let_cap=64, device=torch.device("cpu")).softening == 0.0
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            LetStepper(eng, 0, 1, let_cap=64, device=torch.device("cpu"), softening=bad)
    with pytest.raises(ValueError):
        LetStepper(eng, 0, 1, let_cap=64, device=torch.device("cpu"), softening=0.5)
