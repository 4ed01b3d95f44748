#!/usr/bin/env python3
"""Golden vectors for the stage-2 training forward (`LADIFF._diffusion_process`, ladiff.py:745-813) from the REFERENCE denoiser (build
container only; see make_golden.py): latents noised at one timestep per sample, the rows past each sample's latent count zeroed, the
reference's `LADiffDenoiser` called with `timestep` = a [B] tensor of different values, and `nn.MSELoss` of its output against the noise.

`diffusers` is not installed where this runs, so `noise_scheduler.add_noise` is restated here as diffusers writes it -
`alphas_cumprod[t] ** 0.5 * x0 + (1 - alphas_cumprod[t]) ** 0.5 * noise` in fp32 - over `orc.DDPM().alphas_cumprod`, the table of the
reference's scheduler settings (scaled_linear, 0.00085 .. 0.012, 1000 steps).  Everything after it is the reference's own code.

The values are this file's own draw (`RandomState(2024)`); only the counts and timesteps were chosen by hand.  A recording from other
values gives another loss: batch A's `inst_loss` is 2.00196 for this draw.

Batch A: B = 6, T = 5 - both ends of the schedule, a repeated timestep, a one-latent sample and two full ones.
Batch B: B = 3 - the second batch of the accumulation tests."""
import os, sys
import numpy as np
import torch
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                     # noqa: E402  (reference module builders + ABL; puts the reference on sys.path)
from oracle import ladiff_oracle as orc      # noqa: E402

torch.set_num_threads(8)
T = 5
BATCHES = {"a": ([5, 2, 3, 1, 4, 5], [0, 999, 481, 481, 17, 250]), "b": ([3, 5, 1], [730, 2, 999])}


def add_noise(acp, x0, noise, timesteps):
    """diffusers' DDPMScheduler.add_noise, fp32"""
    a = acp[timesteps] ** 0.5
    b = (1 - acp[timesteps]) ** 0.5
    return a[:, None, None] * x0 + b[:, None, None] * noise


with torch.no_grad():
    den = mg.build_denoiser()
    acp = orc.DDPM().alphas_cumprod
    rs = np.random.RandomState(2024)
    out = {"alphas_cumprod": acp}
    for tag, (counts, steps) in BATCHES.items():
        B = len(counts)
        z = torch.from_numpy(rs.standard_normal((T, B, 256)).astype(np.float32))         # [T,B,256] as vae.encode returns it
        for i, c in enumerate(counts):
            z[c:, i] = 0                                                                 # rows past the count are zero (ladiff_vae.py:258-268)
        noise = torch.from_numpy(rs.standard_normal((B, T, 256)).astype(np.float32))
        text = torch.from_numpy(rs.standard_normal((B, 1, 768)).astype(np.float32))
        ts = torch.tensor(steps, dtype=torch.long)
        cnt = torch.tensor(counts)
        noisy = add_noise(acp, z.permute(1, 0, 2).clone(), noise, ts)                    # ladiff.py:775-776
        for i, c in enumerate(counts):
            noisy[i, c:] = 0                                                             # :779-782
        pred = den(sample=noisy, timestep=ts, encoder_hidden_states=text, lengths=None, return_dict=False, max_iter_elements=cnt)[0]
        loss = torch.nn.MSELoss(reduction="mean")(pred, noise)                           # losses/mld.py:69, :112
        out.update({f"{tag}_z": z, f"{tag}_noise": noise, f"{tag}_text": text, f"{tag}_timesteps": ts, f"{tag}_counts": cnt,
                    f"{tag}_noisy": noisy, f"{tag}_noise_pred": pred, f"{tag}_inst_loss": loss})
        # the oracle's scalar-t forward per sample is the same function (the GPU tests of other shapes take their expected values from it)
        per = torch.cat([orc.denoiser_forward(mg.syn.denoiser_weights(), noisy[i:i + 1], int(steps[i]), text[i:i + 1], cnt[i:i + 1])
                         for i in range(B)])
        same_t = den(sample=noisy, timestep=torch.full((B,), steps[0]), encoder_hidden_states=text, lengths=None, return_dict=False,
                     max_iter_elements=cnt)[0]
        print(f"batch {tag}: inst_loss {loss.item():.6f}  max|noise_pred| {pred.abs().max().item():.2f}  oracle per sample "
              f"{(per - pred).abs().max().item():.2e}  all t = {steps[0]}: {(same_t - pred).abs().max().item():.2f} away")
    mg.save("diffusion_stage", **out)
