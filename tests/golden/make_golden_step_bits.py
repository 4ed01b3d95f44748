#!/usr/bin/env python3
"""Records tests/golden/step_bits_parent.npz (tests/test_gpu_step_bits.py): the pipeline kernel's latents over the branches of the TAIL
stage, from whichever build of the library is given - run it on the GPU with the library of the commit the test is to be pinned to:
    python tests/golden/make_golden_step_bits.py [path/to/libladiff_hip.so] [out.npz]
Every case runs twice; the two runs must agree bit for bit before anything is written.  Per case the file holds a seeded subset of the
prompts (indices and latents) and the SHA-256 of the whole array."""
import os, sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from ladiff_amd import _lib  # noqa: E402
if len(sys.argv) > 1:
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])
import test_gpu_step_bits as S  # noqa: E402

out, nets = {}, S.make_nets()
for sched, B in S.CASES:
    for form in S.FORMS:
        for mode in S.MODES:
            z, again = S.loop_latents(nets, sched, B, form, mode), S.loop_latents(nets, sched, B, form, mode)
            key = S.case_key(sched, B, form, mode)
            assert np.array_equal(z.view(np.uint32), again.view(np.uint32)), f"{key}: two runs of one library differ"
            assert np.isfinite(z).all(), f"{key}: non-finite latents"
            idx = S.subset_index(B).numpy()
            out[key + "__idx"], out[key + "__latents"], out[key + "__sha256"] = idx, z[:, idx], np.array(S.digest(z))
            print(key, z.shape, S.digest(z)[:16], float(np.abs(z).max()), flush=True)
path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "step_bits_parent.npz")
np.savez_compressed(path, **out)
assert os.path.getsize(path) < 1 << 20, f"{path}: {os.path.getsize(path)} bytes - shrink SUBSET"
