"""The loop kernel's host planner (csrc/systolic_plan.hip: workspace carve, block packing, stage table, XCD placement, launch policy) on the CPU:
tests/planner_check.cpp and the planner unit, compiled as plain C++17 with AddressSanitizer + UBSan into a stand-alone program that
runs as a child process.  No GPU, no HIP, nothing loaded into this interpreter."""
import os
import shutil
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "ladiff_amd", "csrc")
# the sanitizer runtimes are linked statically (clang's default; asked of g++), so the program needs nothing from its environment
COMPILERS = [("/opt/rocm/llvm/bin/clang++", []), ("/opt/rocm/lib/llvm/bin/clang++", []), ("clang++", []),
             ("g++", ["-static-libasan", "-static-libubsan"]), ("c++", [])]


def test_planner_properties_under_sanitizers(tmp_path):
    exe = str(tmp_path / "planner_check")
    logs = []
    for cxx, extra in COMPILERS:
        cxx = cxx if os.path.isabs(cxx) else shutil.which(cxx)
        if not cxx or not os.path.exists(cxx):
            continue
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *extra, "-I", CSRC,
               "-x", "c++", os.path.join(ROOT, "tests", "planner_check.cpp"), os.path.join(CSRC, "systolic_plan.hip"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        logs.append(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        if r.returncode == 0:
            break
    else:
        raise AssertionError("no host compiler built the planner check with sanitizers:\n" + "\n".join(logs))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "planner_check: ok" and r.stderr == "", r.stdout + r.stderr
