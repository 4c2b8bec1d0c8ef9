"""tests/sequence_case.py without a GPU: the generator is deterministic, the committed sequences of every precision meet the
coverage condition, and the twin holds the flags of csrc/bh_run_state.hpp after every operation -- tests/run_state_events.cpp
applies, on the header alone, the events each operation fires."""
import os
import re
import subprocess

import pytest

import sequence_case as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-nbody-simulation_amd", "csrc")
EVENTS = os.path.join(ROOT, "tests", "run_state_events.cpp")
IDS = [p.name for p in S.PRECISIONS]


def twins(precision, seq):
    """(operation, the twin's return code, the twin before the call) along a sequence"""
    t = S.Twin(precision)
    for o in seq:
        code = t.predict(o)
        yield o, code, t
        if code == S.OK:
            t.apply(o)


@pytest.mark.parametrize("precision", S.PRECISIONS, ids=IDS)
def test_the_generator_is_deterministic(precision):
    S.random_sequence.cache_clear()
    S.pair_sequences.cache_clear()
    first = S.sequences(precision)
    S.random_sequence.cache_clear()
    S.pair_sequences.cache_clear()
    assert S.sequences(precision) == first
    rnd = [s for i, s in first if i.startswith("random")]
    assert len(rnd) == S.N_RANDOM and all(rnd[i] != rnd[i + 1] for i in range(len(rnd) - 1))
    for _, s in first:
        assert len(s) <= S.SEQ_LEN and s[0] == S.op("upload", "A")
    for s in rnd:
        assert len(s) == S.SEQ_LEN and s[-2:] == (S.op("step", 2), S.op("download"))
        assert any(o.name == "upload" for o in s[1:])                                   # (never the set that is there: _Args, reupload)


@pytest.mark.parametrize("precision", S.PRECISIONS, ids=IDS)
def test_the_coverage_condition(precision):
    seqs = [s for _, s in S.sequences(precision)]
    accepted = []                                    # per sequence: (operation, accepted)
    for s in seqs:
        accepted.append([(o, code == S.OK) for o, code, _ in twins(precision, s)])
    adjacent = {(a.name, b.name) for run in accepted for (a, oa), (b, ob) in zip(run, run[1:]) if oa and ob}
    kinds = S.mover_kinds(precision)
    assert (len(kinds), len(S.OBSERVERS)) == (7 if precision == S.P.F64_EXACT else 8, 16)
    missing = [(k, o) for k in kinds for o in S.OBSERVERS if (k, o) not in adjacent]
    assert missing == [], "a mover kind that no accepted observer directly follows"
    assert [k for k in kinds if (k, "step") not in adjacent] == []
    assert [o for o in S.OBSERVERS if not any((o, p) in adjacent for p in S.OBSERVERS)] == []
    uploads = set()
    for run in accepted:
        there = None
        for o, ok in run:
            if o.name == "upload" and ok:
                uploads.add((there, o.args[0]))
                there = o.args[0]
    assert {(a, b) for a in S.SETS for b in S.SETS if a != b} <= uploads
    refused = {o.name for run in accepted for o, ok in run if not ok}
    assert refused == set(S.REFUSABLE)
    codes = {code for s in seqs for _, code, _ in twins(precision, s)}
    assert codes == {S.OK, S.ERR_ARG, S.ERR_STATE}
    # every value of every argument is used, and set_softening is called with the value that is there
    used = {(o.name, o.args) for s in seqs for o in s}
    assert {(o.name, o.args) for o in S.pool(precision)} <= used
    if precision != S.P.F64_EXACT:
        assert any(o.name == "set_softening" and o.args[0] == t.softening for s in seqs for o, _, t in twins(precision, s))


def test_the_events_program_includes_the_header_alone():
    inc = re.findall(r'#\s*include\s*([<"][^>"]+[>"])', open(EVENTS).read())
    assert inc == ['"bh_run_state.hpp"', "<cstdio>", "<string>", "<iostream>"]


@pytest.fixture(scope="module")
def events_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("run_state_events") / "run_state_events"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), EVENTS])
    return str(exe)


@pytest.mark.parametrize("precision", S.PRECISIONS, ids=IDS)
def test_the_twin_holds_the_flags_of_the_header(precision, events_exe):
    checked = 0
    for name, seq in S.sequences(precision):
        lines, last, want = [], [], []
        for o, code, t in twins(precision, seq):
            ev = S.events(o, t) or ["nop"]
            lines += ev
            last.append(len(lines) - 1)
        t = S.Twin(precision)
        for o in seq:
            if t.predict(o) == S.OK:
                t.apply(o)
            want.append(t.flags())
        r = subprocess.run([events_exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-200:] + r.stderr
        out = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
        assert len(out) == len(lines)
        for i, o in enumerate(seq):
            assert out[last[i]] == want[i], f"{name}: after operation {i}, {o}: the header holds {out[last[i]]}, the twin {want[i]}"
            checked += 1
    assert checked == sum(len(s) for _, s in S.sequences(precision))
