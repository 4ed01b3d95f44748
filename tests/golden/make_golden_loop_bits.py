#!/usr/bin/env python3
"""Records tests/golden/loop_bits_parent.npz (tests/test_gpu_loop_bits.py): the loop kernel's latents on the benchmark shapes, from
whichever build of the library is given - run it on the GPU with the library of the commit the test is to be pinned to:
    python tests/golden/make_golden_loop_bits.py [path/to/libladiff_hip.so] [out.npz]
Every case runs twice; the two runs must agree bit for bit before anything is written.  Per case and arithmetic mode the file holds
a seeded subset of the prompts (indices and latents) and the SHA-256 of the whole array."""
import os, sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from ladiff_amd import _lib  # noqa: E402
if len(sys.argv) > 1:
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])
import test_gpu_loop_bits as T  # noqa: E402

out, nets = {}, T.make_nets()
for case in sorted(T.CASES):
    for mode in T.MODES:
        z, again = T.loop_latents(nets, case, mode), T.loop_latents(nets, case, mode)
        assert np.array_equal(z.view(np.uint32), again.view(np.uint32)), f"{case} {mode}: two runs of one library differ"
        idx = T.subset_index(z.shape[1]).numpy()
        key = f"{case}__{mode}"
        out[key + "__idx"], out[key + "__latents"], out[key + "__sha256"] = idx, z[:, idx], np.array(T.digest(z))
        print(key, z.shape, T.digest(z)[:16], float(np.abs(z).max()), flush=True)
np.savez_compressed(sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "loop_bits_parent.npz"), **out)
