#!/usr/bin/env python3
"""Device time of one `Joints2Feats` call for 128 motions x 197 frames (HIP events around the Python call, median after a dropped
warm-up; `back_to_back_us`: 20 calls between one pair of events, per call - the launches queue up, so this is the kernel where the
single call also shows the host's enqueue), per output row against the kernel's byte floor (264 B read + 1052 B written per row), and
the numpy restatement of the reference per motion on the same box for scale.  Needs the GPU; writes profiles/joints2feats/timing.json (or the path given as first argument)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import joints2feats_ref as ref                                    # noqa: E402
from ladiff_amd import Joints2Feats                               # noqa: E402

if not torch.cuda.is_available():
    sys.exit("joints2feats_timing.py measures on the GPU; none found")
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "joints2feats", "timing.json")
B, L, WARM, REPS = 128, 197, 5, 50
motions = np.stack([ref.motion(L, seed) for seed in range(1, 9)])
x = torch.from_numpy(motions[np.arange(B) % len(motions)]).float().cuda()
tgt = ref.get_offsets_joints(ref.target_pose())
mean, std = np.zeros(263, dtype=np.float32), np.ones(263, dtype=np.float32)
rows = B * (L - 1)
result = {"B": B, "L": L, "rows": rows, "bytes_per_row": 264 + 1052, "warmup": WARM, "repeats": REPS}
for name, op, kw in (("raw", Joints2Feats(), {}), ("normalised", Joints2Feats(mean, std), {"normalize": True}),
                     ("uniform_skeleton", Joints2Feats(target_offsets=tgt), {})):
    times = []
    for i in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        op(x, [L] * B, **kw)
        b.record()
        b.synchronize()
        if i >= WARM:
            times.append(a.elapsed_time(b) * 1e3)
    us = float(np.median(times))
    chained = []
    for i in range(1 + 10):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            op(x, [L] * B, **kw)
        b.record()
        b.synchronize()
        if i >= 1:
            chained.append(a.elapsed_time(b) * 1e3 / 20)
    result[name] = {"call_us_median": round(us, 1), "call_us_min_max": [round(min(times), 1), round(max(times), 1)],
                    "back_to_back_us": round(float(np.median(chained)), 1),
                    "ns_per_row": round(us * 1e3 / rows, 2), "GB_per_s": round(rows * (264 + 1052) / us / 1e3, 1)}
t0 = time.perf_counter()
for m in motions[:4]:
    ref.process_file(m)
result["host_restatement_ms_per_motion"] = round((time.perf_counter() - t0) / 4 * 1e3, 1)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
json.dump(result, open(out_path, "w"), indent=1)
print(json.dumps(result))
