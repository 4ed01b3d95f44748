"""A selection of the GPU suite run against libladiff_hip_bf16.so (the same sources built with -DLADIFF_SPLIT_BF16: every split-mode
kernel has a second instantiation there, on another MFMA and another conversion).

The split format is chosen once per process, so a module-scoped fixture starts ONE fresh child process - `python -m pytest` over the
node ids of tests/bf16_selection.py with LADIFF_TEST_LIB pointing at the bf16-pair library (the hook tests/conftest.py has) - and
reads the per-case outcomes back from the child's junit XML.  Every selected case is a test of its own here, with the child's failure
text.  A child that crashes, times out or reports fewer cases than the list fails every entry with the tail of its output; nothing is
retried.  The selection: per split-mode kernel family the smallest existing cases at which it can still go wrong, and the range cases
(tests/test_gpu_range.py: operands beyond fp16's range, within trained_like.bound(..., split_format=0) of the fp64 oracle).
tests/test_gpu_path.py::test_bf16_pair_flavour_of_the_library stays: it alone goes through `_lib.select_split_format("bf16")` and
LADIFF(precision="bf16x3").

Measured on one MI355X.  pytest's own time for the 117 ids in one process: 24.8 s on the bf16-pair library, 26.2 s for the same ids on
the fp16-pair library (most of it the CPU oracle of each module's first case; the GPU part of every case is milliseconds; measured
with a 5.8 s edit case that has since been swapped for a 1.5 s one, the slowest case left takes 3.5 s).  Worst err / e32 per
family on the bf16-pair library (`pytest -s` prints them; the split bound is 2048 e32 + 1e-6 scale, trained_like.bound(...,
split_format=0)): decoder routing / memory tokens 37.4 (routing 2, ragged), denoiser forward 77.8 (B = 1, T = 1, masked), linear_ca 27.5
(N = 77), sampling loop 91.0 (default form, no guidance, B = 7, frames), encoder 59.7 (T = 3, S = 8, mu), CLIP 45.7 (S = 33 ragged),
range cases 31.0 in split mode (encode x 1e5, latent) and 2.2 in fp32 mode; three-term emulation at most 0.25 of its bound; the
kernel-level range cases 0.02 ... 0.04 of 4 x 2^-16 |A| |W|^T; the split self-attention with V x 3e5 err 3.9 against a bound of 473.
A triage run of the whole suite on this library: profiles/bf16_suite/README.md.

The new tests bite (trial builds of the bf16-pair library, never committed; each run once against the selection):

* bf16 build whose `s16_of` / `split2` clamp at +-65504 (csrc/common.h): 16 of the 117 cases failed - the split-mode range cases of
  the denoiser (5) and the encoder (1), all 8 kernel-level range GEMMs, the split self-attention with V x 3e5, and
  test_split_operands_saturate_instead_of_overflowing; the other 101 passed, among them every case below fp16's range and all
  fp32-mode range cases.  The four split-mode decode range cases passed as well: the decoder projects its memory in fp32 in both
  modes (tests/range_cases.py).  scripts/bf16_flavour_check.py on that build: passed (6.96e-5) - it cannot see this defect.
* bf16 build whose large-M split GEMM (csrc/gemm_big.hip) drops the hi x lo cross term: 44 failed, 73 passed.  Failed: the family's own
  three-term cases (all 5 test_gemm_split_large_m, test_split_products_of_small_operands_per_element[large_m], the 4 large-M range
  GEMMs) and what runs on that kernel (one-launch layer tail 4, decoder routing switch value 5, all 13 sampling-loop cases, all 11 encoder shapes,
  trajectory, DPM-Solver++, edit, per-prompt parameters, the encoder range case); the K-resident GEMM, attention, feed-forward,
  denoiser, CLIP and linear_ca cases passed.  scripts/bf16_flavour_check.py on that build: FAILED too (6.98e-3 against its 1e-3) - this
  kernel serves the decode of its two prompts, so the script alone does catch this one; it names no kernel, the three-term case does."""
import os
import subprocess
import sys
import time
import xml.etree.ElementTree as ET

import pytest

from bf16_selection import SELECTION

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16_LIB = os.path.join("ladiff_amd", "libladiff_hip_bf16.so")
CHILD_TIMEOUT = 600          # seconds; the child takes about a minute (module docstring)


def junit_key(node_id):
    """"tests/test_x.py::test_y[p]" -> ("tests.test_x", "test_y[p]"): classname and name of the case in a junit XML."""
    path, name = node_id.split("::", 1)
    return path[:-3].replace("/", "."), name


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """{"outcomes": {junit key: None (passed) or the failure text}, "crash": None or why no outcome can be trusted}."""
    xml = tmp_path_factory.mktemp("bf16_child") / "junit.xml"
    env = dict(os.environ, LADIFF_TEST_LIB=BF16_LIB)
    cmd = [sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", f"--junitxml={xml}"] + [i for _, i in SELECTION]
    t0 = time.time()
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        out, rc = r.stdout + r.stderr, r.returncode
    except subprocess.TimeoutExpired as e:
        out = "".join(s.decode(errors="replace") if isinstance(s, bytes) else (s or "") for s in (e.stdout, e.stderr))
        rc = f"no exit status: killed after {CHILD_TIMEOUT} s"
    print(f"\n[bf16 flavour] child: {len(SELECTION)} cases, exit status {rc}, {time.time() - t0:.1f} s wall")
    outcomes = {}
    if xml.exists():
        try:
            for case in ET.parse(xml).getroot().iter("testcase"):
                bad = [e for e in case if e.tag in ("failure", "error", "skipped")]
                outcomes[(case.get("classname"), case.get("name"))] = (
                    "\n".join(f"{e.tag}: {e.get('message') or ''}\n{e.text or ''}" for e in bad) if bad else None)
        except ET.ParseError as e:
            outcomes = {}
            out += f"\n(junit XML unreadable: {e})"
    missing = [i for _, i in SELECTION if junit_key(i) not in outcomes]
    crash = None
    if rc not in (0, 1) or missing:              # pytest: 0 = all passed, 1 = some failed; anything else is no test result
        crash = (f"the bf16 child gave no trustworthy result (exit status {rc}, {len(outcomes)} of {len(SELECTION)} cases reported, "
                 f"first missing: {missing[:3]}); the end of its output:\n{out[-3000:]}")
    return {"outcomes": outcomes, "crash": crash}


@pytest.mark.parametrize("family,node_id", SELECTION, ids=[f"{f}::{i.split('::', 1)[1]}" for f, i in SELECTION])
def test_on_the_bf16_pair_library(child, family, node_id):
    assert child["crash"] is None, child["crash"]
    text = child["outcomes"][junit_key(node_id)]
    assert text is None, f"{node_id} on {BF16_LIB} ({family}):\n{text}"
