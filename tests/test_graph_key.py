"""The capture keys of the library's hipGraphs (csrc/graph_key.h: GraphKey, weights_hash, the sampler's and the decode graph's key
builders) on the CPU: tests/graph_key_check.cpp, compiled as plain C++17 with AddressSanitizer + UBSan into a stand-alone program that
runs as a child process.  No GPU, no HIP, nothing loaded into this interpreter."""
import os
import shutil
import subprocess

from conftest import ROOT
from test_planner import COMPILERS, CSRC


def test_graph_key_properties_under_sanitizers(tmp_path):
    exe = str(tmp_path / "graph_key_check")
    logs = []
    for cxx, extra in COMPILERS:
        cxx = cxx if os.path.isabs(cxx) else shutil.which(cxx)
        if not cxx or not os.path.exists(cxx):
            continue
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *extra, "-I", CSRC,
               os.path.join(ROOT, "tests", "graph_key_check.cpp"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        logs.append(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        if r.returncode == 0:
            break
    else:
        raise AssertionError("no host compiler built the graph key check with sanitizers:\n" + "\n".join(logs))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "graph_key_check: ok" and r.stderr == "", r.stdout + r.stderr
