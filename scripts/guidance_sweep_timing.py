"""A guidance sweep, timed in both forms on the same box in the same process:
`python scripts/guidance_sweep_timing.py [prompts=24] [repeats=7] [out.json]`.

  scalar   one `LADIFF.sample` call per scale, P prompts each: every new scale drains the stream and captures the prologue graph again
  batched  ONE call on the P prompts repeated once per scale, with `guidance_scale=` as a per-prompt array (G x P prompts in a launch)

HumanML geometry (263 features, lengths 40 .. 196), synthetic weights, 50-step guided DDIM in the shipped arithmetic (f16x3), scales
1.5, 3.0, 4.5, 6.0, 7.5, text embeddings given.  The two forms alternate (which goes first alternates too); the first round warms plans
and graphs and is dropped; the median wall time of the rest is reported, with every run, as one JSON line."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ladiff_amd import LADIFF, DDIMScheduler, LADiffDenoiser, LADiffVae, synthetic as syn
from ladiff_amd.schema import ABL, DEN_KW, VAE_KW

P = int(sys.argv[1]) if len(sys.argv) > 1 else 24
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
OUT = sys.argv[3] if len(sys.argv) > 3 else None
SCALES = [1.5, 3.0, 4.5, 6.0, 7.5]
G = len(SCALES)
dev = torch.device("cuda", 0)

den = LADiffDenoiser(ABL, **DEN_KW); den.load_state_dict(syn.denoiser_weights())
vae = LADiffVae(ABL, **VAE_KW); vae.load_state_dict(syn.vae_weights(263))
sch = DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                    set_alpha_to_one=False, steps_offset=1)
model = LADIFF(denoiser=den.to(dev).eval(), vae=vae.to(dev).eval(), scheduler=sch, guidance_scale=7.5, num_inference_timesteps=50, eta=0.0,
               precision="f16x3")

rs = np.random.RandomState(2)
lengths = [int(l) for l in rs.randint(40, 197, size=P)]
text = syn.text_embeddings(P, seed=5).to(dev)                       # [2P,1,768], unconditional half first
noise = syn.init_noise(lengths, seed=6).to(dev)
text_all = torch.cat([text[:P].repeat(G, 1, 1), text[P:].repeat(G, 1, 1)])
noise_all, lengths_all = noise.repeat(G, 1, 1), lengths * G
scales_all = [g for g in SCALES for _ in range(P)]


def scalar():
    return torch.cat([model.sample(text, lengths, init_noise=noise, guidance_scale=g)[1] for g in SCALES])


def batched():
    return model.sample(text_all, lengths_all, init_noise=noise_all, guidance_scale=scales_all)[1]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    feats = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, feats


runs = {"scalar": [], "batched": []}
with torch.cuda.stream(torch.cuda.Stream(device=dev)), torch.no_grad():
    for i in range(1 + REPEATS):
        order = (("scalar", scalar), ("batched", batched)) if i % 2 == 0 else (("batched", batched), ("scalar", scalar))
        got = {}
        for name, fn in order:
            wall, got[name] = timed(fn)
            if i:
                runs[name].append(round(wall * 1e3, 3))
        diff = (got["scalar"] - got["batched"]).abs().max().item()     # the same frames either way (other block packing: not the same bits)
        assert torch.isfinite(got["batched"]).all() and diff < 1e-3, diff
model.check()
med = {k: statistics.median(v) for k, v in runs.items()}
line = {"workload": f"guidance sweep: {P} prompts x {G} scales {SCALES}, HumanML geometry, lengths 40-196, DDIM 50, f16x3, synthetic weights",
        "device": torch.cuda.get_device_name(0), "repeats_timed": REPEATS,
        "scalar_one_call_per_scale_ms": med["scalar"], "batched_one_call_ms": med["batched"],
        "motions_per_s": {k: round(P * G / (v * 1e-3), 1) for k, v in med.items()},
        "speedup": round(med["scalar"] / med["batched"], 3), "max_frame_diff": diff, "all_runs_ms": runs}
print(json.dumps(line))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
