"""An edit-strength sweep, timed in both forms on the same box in the same process:
`python scripts/strength_sweep_timing.py [prompts=24] [strengths=0.2,0.4,0.6,0.8,1.0] [repeats=7] [out.json]`.

  sliced   what a caller could do before `source_latents=`: per strength a schedule cut in Python (its own plan, time tables and graphs),
           the noised latents computed in torch and passed as `init_noise` - one `LADIFF.sample` call per strength, P prompts each
  batched  ONE call on the P prompts repeated once per strength with a per-prompt `strength=` array (S x P prompts in a launch): prompts
           that start late ride along frozen until their own start

HumanML geometry (263 features, lengths 40 .. 196), synthetic weights, 50-step guided DDIM in the shipped arithmetic (f16x3), text
embeddings and source latents given.  The two forms alternate (which goes first alternates too); the first round warms plans and graphs
and is dropped; the median wall time of the rest is reported, with every run, as one JSON line.  With ONE strength (e.g. `128 0.3`) the
two forms run the same steps on the same prompts: what is left is the price of the per-prompt form itself."""
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
STRENGTHS = [float(s) for s in (sys.argv[2] if len(sys.argv) > 2 else "0.2,0.4,0.6,0.8,1.0").split(",")]
REPEATS = int(sys.argv[3]) if len(sys.argv) > 3 else 7
OUT = sys.argv[4] if len(sys.argv) > 4 else None
S, N = len(STRENGTHS), 50
dev = torch.device("cuda", 0)
KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
          set_alpha_to_one=False, steps_offset=1)


class SlicedDDIM(DDIMScheduler):
    """The N-step schedule from position `start` on: the cut a caller makes by hand."""

    def __init__(self, start, **kw):
        super().__init__(**kw)
        self.start = start

    def set_timesteps(self, num_inference_steps, device=None):
        super().set_timesteps(N)
        self.timesteps = self.timesteps[self.start:]


den = LADiffDenoiser(ABL, **DEN_KW); den.load_state_dict(syn.denoiser_weights())
vae = LADiffVae(ABL, **VAE_KW); vae.load_state_dict(syn.vae_weights(263))
den, vae = den.to(dev).eval(), vae.to(dev).eval()
make = lambda sch, n: LADIFF(denoiser=den, vae=vae, scheduler=sch, guidance_scale=7.5, num_inference_timesteps=n, eta=0.0, precision="f16x3")
model = make(DDIMScheduler(**KW), N)
starts = [model.scheduler.start_step(s, N) for s in STRENGTHS]
sliced_models = [make(SlicedDDIM(st, **KW), N - st) for st in starts]

rs = np.random.RandomState(2)
lengths = [int(l) for l in rs.randint(40, 197, size=P)]
text = syn.text_embeddings(P, seed=5).to(dev)                       # [2P,1,768], unconditional half first
noise = syn.init_noise(lengths, seed=6).to(dev)                     # [P,5,256]
source = torch.randn(5, P, 256, generator=torch.Generator().manual_seed(7)).to(dev)      # [T,P,256], the layout of the loop's z
text_all = torch.cat([text[:P].repeat(S, 1, 1), text[P:].repeat(S, 1, 1)])
noise_all, lengths_all, source_all = noise.repeat(S, 1, 1), lengths * S, source.repeat(1, S, 1)
strength_all = [s for s in STRENGTHS for _ in range(P)]


def sliced():
    out = []
    for m, st in zip(sliced_models, starts):
        full = DDIMScheduler(**KW)
        full.set_timesteps(N)
        noised = full.add_noise(source.permute(1, 0, 2), noise, full.timesteps[st:st + 1].expand(P))
        out.append(m.sample(text, lengths, init_noise=noised)[1])
    return torch.cat(out)


def batched():
    return model.sample(text_all, lengths_all, init_noise=noise_all, source_latents=source_all, strength=strength_all)[1]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    feats = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, feats


runs = {"sliced": [], "batched": []}
with torch.cuda.stream(torch.cuda.Stream(device=dev)), torch.no_grad():
    for i in range(1 + REPEATS):
        order = (("sliced", sliced), ("batched", batched)) if i % 2 == 0 else (("batched", batched), ("sliced", sliced))
        got = {}
        for name, fn in order:
            wall, got[name] = timed(fn)
            if i:
                runs[name].append(round(wall * 1e3, 3))
        diff = (got["sliced"] - got["batched"]).abs().max().item()     # the same frames either way (other block packing: not the same bits)
        assert torch.isfinite(got["batched"]).all() and diff < 1e-3, diff
model.check()
med = {k: statistics.median(v) for k, v in runs.items()}
steps_run = {"sliced": sum(N - st for st in starts) * P, "batched": (N - min(starts)) * P * S}
line = {"workload": f"strength sweep: {P} prompts x {S} strengths {STRENGTHS} (starts {starts} of {N}), HumanML geometry, lengths 40-196, "
                    "DDIM 50, f16x3, synthetic weights",
        "device": torch.cuda.get_device_name(0), "repeats_timed": REPEATS,
        "sliced_one_call_per_strength_ms": med["sliced"], "batched_one_call_ms": med["batched"],
        "prompt_steps_run": steps_run, "motions_per_s": {k: round(P * S / (v * 1e-3), 1) for k, v in med.items()},
        "speedup": round(med["sliced"] / med["batched"], 3), "max_frame_diff": diff, "all_runs_ms": runs}
print(json.dumps(line))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
