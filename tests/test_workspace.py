"""Workspace layouts (csrc/workspace.h) on the CPU.

1. Every exported size query over a grid of shapes equals tests/golden/workspace_queries.json, recorded from the library as it was
   before the layouts were gathered in one header (DESIGN.md names the commit).  Re-record only when a layout changes on purpose:
   `python tests/test_workspace.py <libladiff_hip.so> tests/golden/workspace_queries.json`.
2. tests/workspace_check.cpp, compiled as plain C++17 with AddressSanitizer + UBSan into a stand-alone program that runs as a child
   process, holds every layout to its properties (order, no overlap, bounds, total = query, null base, rounding, alignment).
No GPU, no HIP call, nothing loaded into this interpreter but the product library's host arithmetic."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_queries.json")
CSRC = os.path.join(ROOT, "ladiff_amd", "csrc")
STEPS = [1, 50, 64, 65, 67, 1000]               # one window | the benchmark's | the longest window and the first schedules past it | DDPM


def grid():
    """(entry, args) pairs: the smallest legal shapes, the regime boundaries of the code, the benchmark's shapes."""
    g = []
    g += [("ladiff_denoiser_tables_floats", (n,)) for n in STEPS]
    g += [("ladiff_denoiser_text_cache_floats", (b2, n, nt)) for b2 in (1, 256) for n in (1, 50, 1000) for nt in (1, 2)]
    g += [("ladiff_denoiser_workspace_bytes", (b2, t, n, nt)) for b2 in (1, 2, 256) for t in (1, 5, 8) for n in STEPS for nt in (1, 2)]
    g += [("ladiff_reverse_workspace_bytes", (b, t, n, nt)) for b in (1, 128, 300) for t in (1, 5) for n in STEPS for nt in (1, 2)]
    g += [("ladiff_reverse_workspace_bytes", (b, 8, 50, 77)) for b in (1, 64, 128)]
    g += [("ladiff_reverse_status_offset_bytes", (b, t, n, 1)) for b, t in ((1, 1), (128, 5)) for n in (1, 50, 1000)]
    g += [("ladiff_linear_cross_attention_workspace_bytes", (b, t, n)) for b in (1, 128) for t in (1, 5) for n in (1, 2, 77)]
    # decoder rows B * F around DEC_SMALL_ROWS = 4096: 64 * 64, 65 * 63 = 4095, 241 * 17 = 4097
    dec = [(1, 1), (1, 224), (8, 60), (64, 64), (65, 63), (241, 17), (64, 196), (128, 196)]
    g += [("ladiff_decoder_workspace_bytes", (b, f, t, 263)) for b, f in dec for t in (1, 5)]
    g += [("ladiff_decoder_workspace_bytes", (128, 196, 5, 251)), ("ladiff_decoder_workspace_bytes", (128, 196, 8, 263))]
    g += [("ladiff_encoder_workspace_bytes", (b, f, t, c)) for b, f in ((1, 1), (8, 60), (128, 196), (3, 208)) for t in (1, 5, 8)
          for c in (1, 251, 263)]
    # CLIP rows around CLIP_SMALL_ROWS = 256 and CLIP_FC2_KPARTS_MAX_ROWS = 8192
    g += [("ladiff_clip_workspace_bytes", a) for a in ((1, 1), (1, 77), (2, 20), (16, 16), (256, 1), (257, 1), (128, 32), (8191, 1),
                                                       (8192, 1), (8193, 1), (128, 64), (128, 77))]
    g += [("ladiff_clip_workspace_bytes_ragged", (b, r)) for b in (1, 4, 128) for r in (1, 4, 128, 255, 256, 257, 2260, 8191, 8192, 8193, 9856)
          if r >= b]
    g += [("ladiff_t2m_movement_workspace_bytes", (b, f, c)) for b in (1, 32) for f in (4, 5, 196, 224) for c in (1, 247, 259)]
    g += [("ladiff_t2m_motion_workspace_bytes", (b, t)) for b in (1, 32, 128) for t in (1, 49, 56)]
    g += [("ladiff_t2m_text_workspace_bytes", (b, l)) for b in (1, 32, 128) for l in (1, 20, 77)]
    return g


def evaluate(cdll):
    rows = []
    for name, args in grid():
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int] * len(args)
        rows.append([name, list(args), int(fn(*args))])
    return rows


def test_queries_equal_the_recorded_values():
    from ladiff_amd import _lib, build
    build.build()
    golden = json.load(open(GOLDEN))
    got = evaluate(ctypes.CDLL(_lib.LIB_PATH))
    assert len(got) == len(golden["rows"]) >= 300
    diff = [(g, w) for g, w in zip(got, golden["rows"]) if g != w]
    assert not diff, f"{len(diff)} queries differ from {golden['recorded_from']} (got, recorded): {diff[:10]}"


# the sanitizer runtimes are linked statically (clang's default; asked of g++), so the program needs nothing from its environment
COMPILERS = [("/opt/rocm/llvm/bin/clang++", []), ("/opt/rocm/lib/llvm/bin/clang++", []), ("clang++", []),
             ("g++", ["-static-libasan", "-static-libubsan"]), ("c++", [])]


def test_layout_properties_under_sanitizers(tmp_path):
    exe = str(tmp_path / "workspace_check")
    logs = []
    for cxx, extra in COMPILERS:
        cxx = cxx if os.path.isabs(cxx) else shutil.which(cxx)
        if not cxx or not os.path.exists(cxx):
            continue
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *extra, "-I", CSRC,
               "-x", "c++", os.path.join(ROOT, "tests", "workspace_check.cpp"), os.path.join(CSRC, "systolic_plan.hip"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        logs.append(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        if r.returncode == 0:
            break
    else:
        raise AssertionError("no host compiler built the workspace check with sanitizers:\n" + "\n".join(logs))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "workspace_check: ok" and r.stderr == "", r.stdout + r.stderr


if __name__ == "__main__":      # record: <library> <output.json> [<commit>]
    rows = evaluate(ctypes.CDLL(os.path.abspath(sys.argv[1])))
    with open(sys.argv[2], "w") as f:
        f.write('{"recorded_from": %s,\n "rows": [\n' % json.dumps(sys.argv[3] if len(sys.argv) > 3 else "unknown"))
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n ]}\n")
    print(len(rows), "rows")
