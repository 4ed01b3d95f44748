#!/usr/bin/env python3
"""Device time of the two joint-metric updates at B = 128, F = 196, J = 22 (HIP events, median after a warm-up) against the same batch
through the numpy restatement on the host, device-to-host copy included.  Needs the GPU; writes profiles/joint_metrics/timing.json
(or the path given as first argument)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import joint_metrics_ref as ref                                   # noqa: E402
from ladiff_amd import ComputeMetrics, MRMetrics                  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("joint_metrics_timing.py measures on the GPU; none found")
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "joint_metrics", "timing.json")
B, F, J, WARM, REPS = 128, 196, 22, 10, 50
rs = np.random.RandomState(0)
rest = rs.uniform(-0.3, 0.3, (J, 3)) + np.array([0.0, 0.9, 0.0])
ref_j = (rest + np.cumsum(rs.standard_normal((B, F, 1, 3)) * 0.02, axis=1) + rs.standard_normal((B, F, J, 3)) * 0.01).astype(np.float32)
rst_j = (ref_j + rs.standard_normal((B, F, J, 3)) * 0.02).astype(np.float32)
lengths = rs.randint(40, F + 1, B).tolist()
lengths[0] = F
d_rst, d_ref = torch.from_numpy(rst_j).cuda(), torch.from_numpy(ref_j).cuda()
result = {"B": B, "F": F, "J": J, "input_MB": round(2 * rst_j.nbytes / 1e6, 1), "warmup": WARM, "repeats": REPS}
for name, m in (("ape_ave", ComputeMetrics(njoints=J, jointstype="humanml3d")), ("mr", MRMetrics(njoints=J, jointstype="humanml3d"))):
    times = []
    for i in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        m.update(d_rst, d_ref, lengths)
        b.record()
        b.synchronize()
        if i >= WARM:
            times.append(a.elapsed_time(b) * 1e3)
    result[f"{name}_update_us_median"] = round(float(np.median(times)), 1)
    result[f"{name}_update_us_min_max"] = [round(min(times), 1), round(max(times), 1)]
torch.cuda.synchronize()
t0 = time.perf_counter()
h_rst, h_ref = d_rst.cpu().numpy(), d_ref.cpu().numpy()
t1 = time.perf_counter()
ref.ape_ave_rows(h_rst, h_ref, lengths, "humanml3d")
t2 = time.perf_counter()
ref.mr_rows(h_rst, h_ref)
t3 = time.perf_counter()
result.update({"host_copy_ms": round((t1 - t0) * 1e3, 2), "host_ape_ave_ms": round((t2 - t1) * 1e3, 1), "host_mr_ms": round((t3 - t2) * 1e3, 1)})
os.makedirs(os.path.dirname(out_path), exist_ok=True)
json.dump(result, open(out_path, "w"), indent=1)
print(json.dumps(result))
