"""DecRoute::post - out_proj + cross-attention + feed-forward as one launch (csrc/dec_post.hip) - and the switch that turns it off
(csrc/graph_key.h: DecSwitches::post_off, an entry of the decode graph's key) on the CPU: tests/dec_post_route_check.cpp, compiled as
plain C++17 with AddressSanitizer + UBSan into a stand-alone program that runs as a child process.  No GPU, no HIP, nothing loaded into
this interpreter."""
import os
import shutil
import subprocess

from conftest import ROOT
from test_planner import COMPILERS, CSRC


def test_dec_post_route_under_sanitizers(tmp_path):
    exe = str(tmp_path / "dec_post_route_check")
    logs = []
    for cxx, extra in COMPILERS:
        cxx = cxx if os.path.isabs(cxx) else shutil.which(cxx)
        if not cxx or not os.path.exists(cxx):
            continue
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *extra, "-I", CSRC,
               os.path.join(ROOT, "tests", "dec_post_route_check.cpp"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        logs.append(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        if r.returncode == 0:
            break
    else:
        raise AssertionError("no host compiler built the route check with sanitizers:\n" + "\n".join(logs))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "dec_post_route_check: ok" and r.stderr == "", r.stdout + r.stderr
