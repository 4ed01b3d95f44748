"""What recording the denoising trajectory costs, on the headline geometry, in one process on one box:
`python scripts/trajectory_timing.py [prompts=128] [frames=196] [passes=20] [out.json]`.

  none      the shipped call: 50-step guided DDIM, `LADIFF.sample`
  latents   the same call with trajectory="latents" (one more 1 KiB store per latent row and step, cloned out per call)
  both      with trajectory="both" (latents and each step's data prediction)
  decode    `decode_trajectory` of the 50 x prompts recorded x0 rows (cut into decodes of `trajectory_decode_samples` samples)

128 prompts of 196 frames (263 features), synthetic weights, guidance 7.5, the shipped arithmetic (f16x3), text embeddings given: one
timed pass = `LADIFF.sample` (denoiser loop + decoder [+ the record's clone]) with a host synchronisation per call.  Each form runs its
passes back to back on a pipe of its own (a graph is replayed only while it is the library's newest instantiation: forms that
alternated call by call would capture their prologue graphs again every time), the unrecorded form first and once more last, so that
a drift of the box over the run shows.  Prints the median pass and the loop's device milliseconds per form as one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from ladiff_amd import LADIFF, DDIMScheduler, LADiffDenoiser, LADiffVae, synthetic as syn
from ladiff_amd.schema import ABL, DEN_KW, VAE_KW

P = int(sys.argv[1]) if len(sys.argv) > 1 else 128
F = int(sys.argv[2]) if len(sys.argv) > 2 else 196
PASSES = int(sys.argv[3]) if len(sys.argv) > 3 else 20
OUT = sys.argv[4] if len(sys.argv) > 4 else None
WARMUP = 3
STEPS = 50
dev = torch.device("cuda", 0)

den = LADiffDenoiser(ABL, **DEN_KW); den.load_state_dict(syn.denoiser_weights())
vae = LADiffVae(ABL, **VAE_KW); vae.load_state_dict(syn.vae_weights(263))
den, vae = den.to(dev).eval(), vae.to(dev).eval()
KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
lengths = [F] * P
text = syn.text_embeddings(P).to(dev)
noise = syn.init_noise(lengths).to(dev)
FORMS = (("none", None), ("latents", "latents"), ("both", "both"), ("none_again", None))


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


with torch.cuda.stream(torch.cuda.Stream(device=dev)), torch.no_grad():
    pipes = {name: LADIFF(denoiser=den, vae=vae, scheduler=DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, **KW),
                          guidance_scale=7.5, num_inference_timesteps=STEPS, eta=0.0, precision="f16x3") for name, _ in FORMS}
    walls, loops = {n: [] for n, _ in FORMS}, {n: [] for n, _ in FORMS}
    z_of, traj = {}, None
    for name, kind in FORMS:
        pipe = pipes[name]
        for i in range(WARMUP + PASSES):                          # the first passes warm plans, graphs and the allocator
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe.sample(text, lengths, init_noise=noise, **({} if kind is None else {"trajectory": kind}))
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            assert pipe.loop_status() == (0, 0) and pipe.last_loop()[0]
            z_of[name] = out[0]
            if kind == "both":
                traj = out[2]
            if i >= WARMUP:
                walls[name].append(wall)
                loops[name].append(pipe.loop_ms())
    assert torch.equal(z_of["latents"], z_of["none"]) and torch.equal(z_of["both"], z_of["none"])      # recording changes no bit
    assert torch.equal(traj["latents"][-1], z_of["none"])
    rows = [{"form": name, "pass_ms_median": round(1e3 * median(walls[name]), 3), "pass_ms_min": round(1e3 * min(walls[name]), 3),
             "pass_ms_max": round(1e3 * max(walls[name]), 3), "loop_ms_median": round(median(loops[name]), 3),
             "loop_ms_min": round(min(loops[name]), 3), "loop_ms_max": round(max(loops[name]), 3)} for name, _ in FORMS]
    dec = []
    pipe = pipes["both"]
    for i in range(WARMUP + PASSES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames = pipe.decode_trajectory(traj["x0"], lengths)
        torch.cuda.synchronize()
        if i >= WARMUP:
            dec.append(time.perf_counter() - t0)
    assert tuple(frames.shape) == (STEPS, P, F, 263) and torch.isfinite(frames).all()
base = rows[0]
for r in rows:
    r["pass_over_none"] = round(r["pass_ms_median"] / base["pass_ms_median"], 4)
    r["loop_over_none"] = round(r["loop_ms_median"] / base["loop_ms_median"], 4)
    print(f"# {r['form']:8s} pass {r['pass_ms_median']:8.3f} ms (x{r['pass_over_none']:.3f})  loop {r['loop_ms_median']:8.3f} ms (x{r['loop_over_none']:.3f})")
decode = {"samples": STEPS * P, "samples_per_decode": int(pipe.trajectory_decode_samples), "ms_median": round(1e3 * median(dec), 3),
          "ms_min": round(1e3 * min(dec), 3), "ms_max": round(1e3 * max(dec), 3)}
print(f"# decode_trajectory of {decode['samples']} samples: {decode['ms_median']:.3f} ms")
line = {"workload": f"{P} prompts x {F} frames, 263 features, DDIM-{STEPS}, guidance 7.5, f16x3, synthetic weights",
        "device": torch.cuda.get_device_name(0), "passes_timed": PASSES, "warmup": WARMUP, "last_loop": list(pipe.last_loop()),
        "trajectory_bytes_per_kind": STEPS * P * 5 * 1024, "rows": rows, "decode_trajectory": decode}
print(json.dumps(line))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
