#!/usr/bin/env python3
"""Golden values for `MMMetrics` from the REFERENCE's `metrics/utils.py:calculate_multimodality_np` (numpy / scipy only).
Run where the reference is checked out: `python tests/golden/make_golden_mm.py path/to/reference`; the fixture holds arrays only: the
embeddings, the two index draws the reference made, its result on the float64 array and its result on the float32 array."""
import importlib.util, os, sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = os.path.join(sys.argv[1], "src", "ladiff", "models")

spec = importlib.util.spec_from_file_location("ref_metric_utils", f"{REF}/metrics/utils.py")
mutil = importlib.util.module_from_spec(spec); spec.loader.exec_module(mutil)


def record(act, times, seed):
    """The reference draws from numpy's global generator: seed it, replay the two draws, then let it compute from the same state."""
    np.random.seed(seed)
    first = np.random.choice(act.shape[1], times, replace=False)
    second = np.random.choice(act.shape[1], times, replace=False)
    np.random.seed(seed)
    value = mutil.calculate_multimodality_np(act, times)
    return first, second, value


out = {}
rs = np.random.RandomState(17)
for tag, shape, times, seed in (("main", (12, 30, 512), 10, 101), ("edge", (1, 11, 512), 10, 102)):
    centre = rs.standard_normal((shape[0], 1, shape[2])).astype(np.float32) * 4.0        # prompts apart, repeats around them
    act32 = (centre + rs.standard_normal(shape).astype(np.float32) * np.float32(1.5)).astype(np.float32)
    first, second, v64 = record(act32.astype(np.float64), times, seed)
    f2, s2, v32 = record(act32, times, seed)
    assert np.array_equal(first, f2) and np.array_equal(second, s2)
    out.update({f"{tag}_act": act32, f"{tag}_first": first, f"{tag}_second": second, f"{tag}_times": np.array(times),
                f"{tag}_value64": np.array(v64, dtype=np.float64), f"{tag}_value32": np.array(v32, dtype=np.float32)})
    print(tag, shape, times, repr(v64), repr(v32), type(v32))
np.savez_compressed(os.path.join(HERE, "mm_metrics.npz"), **out)
