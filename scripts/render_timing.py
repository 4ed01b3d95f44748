#!/usr/bin/env python3
"""Device time of the renderer at the headline batch - 128 motions x 196 frames as 256 x 256 uint8 animation frames, and their 128 pose
strips - each beside a hipMemsetAsync of the same output bytes in the same process (the floor of a write-only kernel), and the host side
of one `animate` call for scale: the device-to-host copy of one motion's frames and their GIF encoding.

The frames are rendered in TWO requests of 64 motions (2.47 GB each) into one reused buffer: one request of 128 (4.93 GB) is below
`MotionRenderer.max_render_bytes` too, but two keep the timing buffer and its memset twin inside a few GB of a shared card.  HIP events
around each call, median after dropped warm-ups.  Needs the GPU; writes profiles/render/timing.json (or the path given as first argument)."""
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import render_ref as ref                                          # noqa: E402
from ladiff_amd import MotionRenderer, save_animation             # noqa: E402

if not torch.cuda.is_available():
    sys.exit("render_timing.py measures on the GPU; none found")
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "render", "timing.json")
B, L, H, W, HALF, WARM, REPS = 128, 196, 256, 256, 64, 2, 7
hip = ctypes.CDLL("libamdhip64.so")
hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
motions = np.stack([ref.motion(L, 22, seed, travel=1.0 + seed) for seed in range(8)])
x = torch.from_numpy(motions[np.arange(B) % len(motions)]).float().cuda()
r = MotionRenderer(22, size=(H, W))


def timed(fn, warm=WARM, reps=REPS):
    times = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warm:
            times.append(a.elapsed_time(b))
    return float(np.median(times)), [round(min(times), 3), round(max(times), 3)]


def memset(t):
    assert hip.hipMemsetAsync(t.data_ptr(), 0, t.numel() * t.element_size(), torch.cuda.current_stream().cuda_stream) == 0


def run(kind, **kw):
    """The whole renderer call (allocation of the output included), then the same bytes as a memset."""
    op = r if kind == "frames" else r.strip
    out = op(x[:HALF] if kind == "frames" else x, **kw)
    nbytes = out.numel() * out.element_size() * (2 if kind == "frames" else 1)
    ms, span = timed((lambda: (op(x[:HALF], **kw), op(x[HALF:], **kw))) if kind == "frames" else (lambda: op(x, **kw)))
    floor, fspan = timed((lambda: (memset(out), memset(out))) if kind == "frames" else (lambda: memset(out)))
    return {"output_bytes": nbytes, "ms_median": round(ms, 3), "ms_min_max": span, "GB_per_s": round(nbytes / ms / 1e6, 1),
            "memset_ms_median": round(floor, 3), "memset_ms_min_max": fspan, "ratio_to_memset": round(ms / floor, 2)}


result = {"B": B, "L": L, "H": H, "W": W, "warmup": WARM, "repeats": REPS, "frames_split": f"2 requests of {HALF} motions",
          "frames_uint8": run("frames"), "strip_uint8": run("strip", n_poses=8)}
result["frames_uint8"]["us_per_image"] = round(result["frames_uint8"]["ms_median"] * 1e3 / (B * L), 3)
# the host side of one animate call, one motion: the copy and the encoding dominate whatever the kernel costs
one = r(x[0])
torch.cuda.synchronize()
t0 = time.perf_counter()
host = one.cpu()
t1 = time.perf_counter()
with tempfile.TemporaryDirectory() as d:
    save_animation(host, os.path.join(d, "0.gif"))
    t2 = time.perf_counter()
    gif_bytes = os.path.getsize(os.path.join(d, "0.gif"))
result["animate_host_side_one_motion"] = {"frames": L, "device_to_host_ms": round((t1 - t0) * 1e3, 2), "gif_encode_ms": round((t2 - t1) * 1e3, 1),
                                          "gif_bytes": gif_bytes}
os.makedirs(os.path.dirname(out_path), exist_ok=True)
json.dump(result, open(out_path, "w"), indent=1)
print(json.dumps(result))
