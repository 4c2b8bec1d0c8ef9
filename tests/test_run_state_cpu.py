"""csrc/bh_run_state.hpp -- the engine's record of what is current and its named events -- compiles with the plain host
compiler, includes nothing of HIP, and gives the accepted and refused calls of tests/test_gpu_split.py's state-rule tests when
tests/run_state_replay.cpp replays them on the header alone; the quiet scope restores both of its groups byte for byte."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-nbody-simulation_amd", "csrc")
HEADER = os.path.join(CSRC, "bh_run_state.hpp")
REPLAY = os.path.join(ROOT, "tests", "run_state_replay.cpp")


def test_header_is_hip_free():
    src = open(HEADER).read()
    assert not re.search(r'#\s*include\s*[<"]hip/|__global__|__device__|hipStream', src)
    assert re.findall(r'#\s*include\s*([<"][^>"]+[>"])', src) == ["<cstdint>"]
    assert re.findall(r'#\s*include\s*([<"][^>"]+[>"])', open(REPLAY).read()) == ['"bh_run_state.hpp"', "<cstdio>", "<string>"]


def test_replayed_call_sequences(tmp_path):
    exe = tmp_path / "run_state_replay"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), REPLAY])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "0 failed checks"


def test_the_engine_writes_the_facts_through_events_only():
    """No assignment to a member of the three structs anywhere in the engine unit: the events of the header are the writers."""
    src = open(os.path.join(CSRC, "bh_engine.hip")).read() + open(os.path.join(CSRC, "bh_queries_host.hpp")).read()
    hits = re.findall(r"\b(?:is|carry|last)\.\w+\s*(?:[-+|&]?=(?!=)|\+\+|--)", src)
    assert hits == [], hits
