"""One multimodality pass, timed in both forms on the same box in the same process:
`python scripts/mm_pass_timing.py [prompts=100] [repeats=30] [passes=2] [out.json]`.

  literal  the reference's form: one `t2m_eval` call per prompt with `datamodule.is_mm` set (30 rows per call)
  batched  `LADIFF.mm_eval` on all prompts at once (launches of 10 prompts x 30 repeats)

HumanML geometry (263 features, lengths 40 .. 196), synthetic weights, 50-step guided DDIM in the shipped arithmetic (f16x3), the
12-layer CLIP text tower on word-hash token ids.  Prints motions/s of both forms and the per-stage device times (HIP events around each
stage on the pass's stream; a stage's time includes the gaps the host leaves inside it) as one JSON line."""
import json
import os
import sys
import time
import zlib
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ladiff_amd import (LADIFF, DDIMScheduler, LADiffDenoiser, LADiffVae, MldTextEncoder, MotionEncoderBiGRUCo, MovementConvEncoder,
                        TextEncoderBiGRUCo, synthetic as syn)
from ladiff_amd.schema import ABL, DEN_KW, VAE_KW

P = int(sys.argv[1]) if len(sys.argv) > 1 else 100
R = int(sys.argv[2]) if len(sys.argv) > 2 else 30
PASSES = int(sys.argv[3]) if len(sys.argv) > 3 else 2
OUT = sys.argv[4] if len(sys.argv) > 4 else None
dev = torch.device("cuda", 0)


class WordHashTokenizer:
    """CLIP's framing (BOS 49406, EOS 49407 = the largest id, 77 positions) around one id per word: host string work only."""
    model_max_length = 77

    def __call__(self, texts, **kw):
        ids = np.zeros((len(texts), 77), dtype=np.int64)
        for i, t in enumerate(texts):
            words = [1 + zlib.crc32(w.encode()) % 49000 for w in t.split()][:75]
            row = [49406] + words + [49407]
            ids[i, :len(row)] = row
        return {"input_ids": torch.from_numpy(ids)}


den = LADiffDenoiser(ABL, **DEN_KW); den.load_state_dict(syn.denoiser_weights())
vae = LADiffVae(ABL, **VAE_KW); vae.load_state_dict(syn.vae_weights(263))
enc = MldTextEncoder(tokenizer=WordHashTokenizer(), precision="f16x3")
enc.text_model.load_state_dict(syn.clip_weights(), strict=True)
mv, mo, tx = syn.t2m_weights(263)
move = MovementConvEncoder(259, 512, 512); move.load_state_dict(mv)
motion = MotionEncoderBiGRUCo(512, 1024, 512); motion.load_state_dict(mo)
text = TextEncoderBiGRUCo(300, 15, 512, 512); text.load_state_dict(tx)
rs = np.random.RandomState(2)
mean = torch.from_numpy(rs.standard_normal(263).astype(np.float32)) * 0.1
std = torch.from_numpy(rs.uniform(0.5, 1.5, 263).astype(np.float32))
dm = SimpleNamespace(renorm4t2m=lambda f: (f - mean.to(f.device)) / std.to(f.device), mean=mean, std=std, njoints=22, is_mm=False,
                     feats2joints=None)
sch = DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                    set_alpha_to_one=False, steps_offset=1)
model = LADIFF(None, dm, denoiser=den.to(dev).eval(), vae=vae.to(dev).eval(), scheduler=sch, guidance_scale=7.5,
               num_inference_timesteps=50, eta=0.0, text_encoder=enc.to(dev), precision="f16x3", mm_num_repeats=R)
model.set_t2m_evaluators(text.to(dev), move.to(dev), motion.to(dev), unit_len=4)

lengths = [int(l) for l in rs.randint(40, 197, size=P)]
words = "a person walks runs jumps forward backward slowly quickly then turns left right and sits down waves both hands".split()
texts = [" ".join(rs.choice(words, size=rs.randint(4, 16))) + f" {i}" for i in range(P)]
gen = torch.Generator().manual_seed(3)


def one_prompt_batch(i):
    m = torch.randn(1, lengths[i], 263, generator=gen)
    return {"text": [texts[i]], "length": [lengths[i]], "motion": m, "word_embs": torch.randn(1, 20, 300, generator=gen),
            "pos_ohot": torch.nn.functional.one_hot(torch.randint(0, 15, (1, 20), generator=gen), 15).float(),
            "text_len": torch.tensor([12])}


batches = [one_prompt_batch(i) for i in range(P)]
events = {}


def staged(name, fn):
    def wrapped(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*a, **k)
        e1.record()
        events.setdefault(name, []).append((e0, e1))
        return out
    return wrapped


model.text_encoder.forward = staged("text_tower", model.text_encoder.forward)
model._diffusion_reverse = staged("loop", model._diffusion_reverse)
model.vae.decode = staged("decode", model.vae.decode)
model.t2m_moveencoder.forward = staged("evaluators", model.t2m_moveencoder.forward)
model.t2m_motionencoder.forward = staged("evaluators", model.t2m_motionencoder.forward)
model.t2m_textencoder.forward = staged("evaluators", model.t2m_textencoder.forward)


def literal():
    dm.is_mm = True
    try:
        return torch.stack([model.t2m_eval(b)["lat_rm"] for b in batches])
    finally:
        dm.is_mm = False


def batched():
    return model.mm_eval({"text": texts, "length": lengths})["lat_rm"]


def measure(fn):
    runs = []
    for i in range(1 + PASSES):                                  # the first pass warms plans, graphs and the allocator
        events.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lat = fn()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        stages = {k: round(sum(a.elapsed_time(b) for a, b in v), 3) for k, v in events.items()}
        calls = {k: len(v) for k, v in events.items()}
        assert lat.shape == (P, R, 512) and torch.isfinite(lat).all()
        if i:
            runs.append({"wall_s": round(wall, 4), "motions_per_s": round(P * R / wall, 1), "stage_device_ms": stages, "stage_calls": calls})
    return min(runs, key=lambda r: r["wall_s"]), runs


with torch.cuda.stream(torch.cuda.Stream(device=dev)), torch.no_grad():
    lit_best, lit_runs = measure(literal)
    bat_best, bat_runs = measure(batched)
model.check()
line = {"workload": f"multimodality pass: {P} prompts x {R} repeats, HumanML geometry, lengths 40-196, DDIM 50, f16x3, synthetic weights",
        "device": torch.cuda.get_device_name(0), "passes_timed": PASSES,
        "literal_one_t2m_eval_per_prompt": lit_best, "batched_mm_eval": bat_best,
        "speedup": round(lit_best["wall_s"] / bat_best["wall_s"], 3),
        "launches_batched": len(model.last_mm_launches), "all_runs": {"literal": lit_runs, "batched": bat_runs}}
print(json.dumps(line))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
