"""What fewer solver steps buy in throughput, on the headline geometry, in one process on one box:
`python scripts/solver_steps_timing.py [prompts=128] [frames=196] [passes=10] [out.json]`.

  ddim-50   the shipped schedule: 50-step guided DDIM
  dpm-N     DPMSolverMultistepScheduler (DPM-Solver++(2M), final_sigmas_type="zero") at N = 10, 15, 20, 25, 50 steps

128 prompts of 196 frames (263 features), synthetic weights, guidance 7.5, the shipped arithmetic (f16x3), text embeddings given: one
timed pass = `LADIFF.sample` (denoiser loop + decoder) with a host synchronisation per call.  Prints motions/s and the loop's device
milliseconds per schedule as one JSON line.  THROUGHPUT ONLY: no trained checkpoint is involved, so nothing here says what motion
quality a step count gives."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from ladiff_amd import LADIFF, DDIMScheduler, DPMSolverMultistepScheduler, LADiffDenoiser, LADiffVae, synthetic as syn
from ladiff_amd.schema import ABL, DEN_KW, VAE_KW

P = int(sys.argv[1]) if len(sys.argv) > 1 else 128
F = int(sys.argv[2]) if len(sys.argv) > 2 else 196
PASSES = int(sys.argv[3]) if len(sys.argv) > 3 else 10
OUT = sys.argv[4] if len(sys.argv) > 4 else None
WARMUP = 3
dev = torch.device("cuda", 0)

den = LADiffDenoiser(ABL, **DEN_KW); den.load_state_dict(syn.denoiser_weights())
vae = LADiffVae(ABL, **VAE_KW); vae.load_state_dict(syn.vae_weights(263))
den, vae = den.to(dev).eval(), vae.to(dev).eval()
KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
lengths = [F] * P
text = syn.text_embeddings(P).to(dev)
noise = syn.init_noise(lengths).to(dev)


def measure(name, scheduler, steps):
    pipe = LADIFF(denoiser=den, vae=vae, scheduler=scheduler, guidance_scale=7.5, num_inference_timesteps=steps, eta=0.0,
                  precision="f16x3")
    walls, loops = [], []
    for i in range(WARMUP + PASSES):                              # the first passes warm plans, graphs and the allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        z, feats = pipe.sample(text, lengths, init_noise=noise)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        if i >= WARMUP:
            walls.append(wall)
            loops.append(pipe.loop_ms())
    assert torch.isfinite(feats).all() and pipe.loop_status() == (0, 0) and pipe.last_loop()[0]
    walls.sort(); loops.sort()
    med = walls[len(walls) // 2]
    return {"schedule": name, "steps": steps, "motions_per_s": round(P / med, 1), "pass_ms_median": round(1e3 * med, 3),
            "pass_ms_min": round(1e3 * walls[0], 3), "pass_ms_max": round(1e3 * walls[-1], 3), "loop_ms_median": round(loops[len(loops) // 2], 3)}


with torch.cuda.stream(torch.cuda.Stream(device=dev)), torch.no_grad():
    rows = [measure("ddim-50", DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, **KW), 50)]
    for n in (10, 15, 20, 25, 50):
        rows.append(measure(f"dpm-{n}", DPMSolverMultistepScheduler(**KW), n))
base = rows[0]["motions_per_s"]
for r in rows:
    r["over_ddim_50"] = round(r["motions_per_s"] / base, 3)
    print(f"# {r['schedule']:8s} {r['motions_per_s']:9.1f} motions/s  pass {r['pass_ms_median']:7.3f} ms  loop {r['loop_ms_median']:7.3f} ms  "
          f"x{r['over_ddim_50']:.2f} of ddim-50")
line = {"workload": f"{P} prompts x {F} frames, 263 features, guidance 7.5, f16x3, synthetic weights; throughput only, no quality claim",
        "device": torch.cuda.get_device_name(0), "passes_timed": PASSES, "warmup": WARMUP, "rows": rows}
print(json.dumps(line))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
