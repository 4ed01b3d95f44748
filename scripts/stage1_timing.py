"""One `t2m_eval` batch in stage "vae" against the same batch in stage "diffusion", same box, same process:
`python scripts/stage1_timing.py [batch=64] [frames=196] [passes=5] [out.json]`.

HumanML geometry (263 features), synthetic weights, DVAE on (PERCENTAGE_NOISED 0.33), 50-step guided DDIM for the diffusion stage in the
shipped arithmetic (f16x3), a stub text encoder (a fixed row per string) so that both stages time the same evaluator tail.  Two warm-up
calls per stage, then HIP events around each call on the current stream (a call's time includes the gaps the host leaves inside it);
prints the median per stage as one JSON line."""
import copy
import json
import os
import sys
import zlib
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ladiff_amd import (LADIFF, DDIMScheduler, LADiffDenoiser, LADiffVae, MotionEncoderBiGRUCo, MovementConvEncoder, TextEncoderBiGRUCo,
                        synthetic as syn)
from ladiff_amd.schema import ABL, DEN_KW, VAE_KW

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
F = int(sys.argv[2]) if len(sys.argv) > 2 else 196
PASSES = int(sys.argv[3]) if len(sys.argv) > 3 else 5
OUT = sys.argv[4] if len(sys.argv) > 4 else None
dev = torch.device("cuda", 0)


def text_encoder(texts):
    rows = [torch.randn(768, generator=torch.Generator().manual_seed(zlib.crc32(t.encode()))) for t in texts]
    return torch.stack(rows).unsqueeze(1).to(dev)


abl = copy.copy(ABL)
abl.DVAE, abl.PERCENTAGE_NOISED = True, 0.33
den = LADiffDenoiser(ABL, **DEN_KW); den.load_state_dict(syn.denoiser_weights(), strict=True)
vae = LADiffVae(abl, **VAE_KW); vae.load_state_dict(syn.vae_weights(263), strict=True)
mv, mo, tx = syn.t2m_weights(263)
move = MovementConvEncoder(259, 512, 512); move.load_state_dict(mv, strict=True)
motion = MotionEncoderBiGRUCo(512, 1024, 512); motion.load_state_dict(mo, strict=True)
text = TextEncoderBiGRUCo(300, 15, 512, 512); text.load_state_dict(tx, strict=True)
rs = np.random.RandomState(2)
mean, std = torch.from_numpy(rs.standard_normal(263).astype(np.float32)) * 0.1, torch.from_numpy(rs.uniform(0.5, 1.5, 263).astype(np.float32))
dm = SimpleNamespace(renorm4t2m=lambda f: f, mean=mean, std=std, njoints=22, is_mm=False, feats2joints=None)
gen = torch.Generator().manual_seed(1)
batch = {"text": [f"motion number {i}" for i in range(B)], "length": [F] * B, "motion": torch.randn(B, F, 263, generator=gen).to(dev),
         "word_embs": torch.randn(B, 12, 300, generator=gen), "pos_ohot": torch.nn.functional.one_hot(torch.randint(0, 15, (B, 12), generator=gen), 15).float(),
         "text_len": torch.tensor(sorted(torch.randint(2, 13, (B,), generator=gen).tolist(), reverse=True))}

result = {"batch": B, "frames": F, "passes": PASSES}
for stage in ("vae", "diffusion"):
    model = LADIFF(None, dm, denoiser=den.to(dev).eval(), vae=vae.to(dev).eval(),
                   scheduler=DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                           clip_sample=False, set_alpha_to_one=False, steps_offset=1),
                   guidance_scale=7.5, num_inference_timesteps=50, eta=0.0, text_encoder=text_encoder, precision="f16x3", stage=stage)
    model.set_t2m_evaluators(text.to(dev), move.to(dev), motion.to(dev), unit_len=4)
    for _ in range(2):
        model.t2m_eval(batch)
    times = []
    for _ in range(PASSES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = model.t2m_eval(batch)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    assert torch.isfinite(out["m_rst"]).all()
    result[stage + "_ms"] = float(np.median(times))
    result[stage + "_ms_all"] = [round(t, 3) for t in times]
print(json.dumps(result))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f)
