"""Helper of the static kernel checks (no test in here): a unit of csrc/ compiled to gfx950 assembly, once per process,
and the per-kernel records of the code object's metadata notes."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-nbody-simulation_amd", "csrc")
UNIT_FLAGS = {"bh_engine.hip": ["-ffp-contract=off"], "bh_walk_fast.hip": []}     # as build.py compiles them


@functools.lru_cache(maxsize=None)
def assembly(unit, diagnostics=False):
    """(assembly text, compiler stderr) of csrc/<unit>; diagnostics: with the build's -Wall instead of -w."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    warn = ["-Wall", "-Wno-unused-function"] if diagnostics else ["-w"]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit + ".s")
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", *UNIT_FLAGS[unit], "-S", "--cuda-device-only",
                            *warn, "-o", out, os.path.join(CSRC, unit)], cwd=CSRC, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        with open(out) as fh:
            return fh.read(), r.stderr


def kernels(text, name=r"\S+"):
    """kernel symbol -> {sgpr, vgpr, sgpr_spill, vgpr_spill, scratch, dynamic_stack} of every kernel whose symbol matches
    the regular expression `name`."""
    res = {}
    for m in re.finditer(r"\.name:\s+(" + name + r")\n", text):
        meta = text[m.start():m.start() + 3000]
        if ".private_segment_fixed_size" not in meta:
            continue
        val = lambda key: int(re.search(key + r":\s+(\d+)", meta).group(1))
        res[m.group(1)] = {
            "sgpr": val(r"\.sgpr_count"), "vgpr": val(r"\.vgpr_count"), "sgpr_spill": val(r"\.sgpr_spill_count"),
            "vgpr_spill": val(r"\.vgpr_spill_count"), "scratch": val(r"\.private_segment_fixed_size"),
            "dynamic_stack": re.search(r"\.uses_dynamic_stack:\s+(\w+)", meta).group(1),
        }
    return res
