"""The pipeline kernel's TAIL stage, bit for bit, on everything the end of a step can do: arrays recorded from the library of the commit
BEFORE the step's arithmetic moved into csrc/step_rule.h (guidance, noise selection and the scheduler update, shared by the three
tails).  tests/test_gpu_loop_bits.py pins DDIM only (k_noise = 0, no x0_prev, scalar guidance); here are the other branches:

    ddpm_gen     DDPM, noise drawn by the device generator from a fixed `noise_seed`
    ddim_eta     DDIM eta = 0.5 with a `step_noise` tensor
    dpm2m        DPM-Solver++(2M): the k_m m1 term, x0_prev (6 steps = orders 1, 2, 2, 2, 2, 1)
    ddpm_prompts DDPM with a guidance scale, a noise key and a prompt index per prompt            (7 prompts only)
    ddim_plain   DDIM without guidance: a block is a unit of its own                            (7 prompts only)

T = 5, 6 steps, synthetic weights.  7 prompts of latent counts 1 .. 5: blocks with pairs of several prompts, padding rows, two units
(a tail owns one: tail_loop does not prefetch).  43 prompts of mixed counts: more than NTAIL units, tail_loop prefetches and m1 travels
in Pay.  Each on 16-row blocks, on 16-row blocks with the look-ahead instantiation forced in (ladiff_debug_set_loop_thresholds(1, -1)),
and on 32-row blocks, in both arithmetic modes.  The fixture (tests/golden/step_bits_parent.npz, written by
tests/golden/make_golden_step_bits.py on the GPU with the parent commit's library) keeps a seeded subset of SUBSET prompts per case and
the SHA-256 of the whole array; the tolerance is zero."""
import hashlib

import numpy as np
import pytest
import torch

from ladiff_amd import LADIFF, DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, LADiffDenoiser, LADiffVae, _lib, synthetic as syn
from test_abi import ABL, DEN_KW, VAE_KW

DEV = "cuda:0"
T, STEPS = 5, 6
SUBSET, SUBSET_SEED = 4, 0
SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
LENS = {7: [48, 91, 134, 192, 196, 38, 96],                                               # latent counts 1 .. 5
        43: [max(1, min(196, 48 * ((i % T) + 1) - 5 * (i % 3))) for i in range(43)]}      # as tests/test_gpu_dpm_solver.py:mixed_lengths
SCHEDULES = {"ddpm_gen": (7, 43), "ddim_eta": (7, 43), "dpm2m": (7, 43), "ddpm_prompts": (7,), "ddim_plain": (7,)}
CASES = [(s, B) for s in sorted(SCHEDULES) for B in SCHEDULES[s]]
FORMS = ("pipeline16", "pipeline16_look_ahead", "pipeline32")
MODES = ("f16x3", "fp32")


def subset_index(n):
    return torch.randperm(n, generator=torch.Generator().manual_seed(SUBSET_SEED))[:SUBSET].sort().values


def make_nets():
    den = LADiffDenoiser(ABL, **DEN_KW); den.load_state_dict(syn.denoiser_weights(), strict=True)
    vae = LADiffVae(ABL, **VAE_KW); vae.load_state_dict(syn.vae_weights(263), strict=True)
    return den.to(DEV).eval(), vae.to(DEV).eval()


def loop_latents(nets, sched, B, form, mode):
    """[T, B, 256] latents of one 6-step loop through the pipeline kernel, as a numpy float32 array."""
    den, vae = nets
    lens = LENS[B]
    text, kw, eta, scale = syn.text_embeddings(B, seed=900 + B).to(DEV), {}, 0.0, 7.5
    if sched == "ddpm_gen":
        sch, kw = DDPMScheduler(variance_type="fixed_small", clip_sample=False, **SCHED_KW), dict(noise_seed=1234 + B)
    elif sched == "ddim_eta":
        sch, eta = DDIMScheduler(set_alpha_to_one=False, steps_offset=1, clip_sample=False, **SCHED_KW), 0.5
        kw = dict(step_noise=torch.randn(STEPS, B, T, 256, generator=torch.Generator().manual_seed(50 + B)).to(DEV))
    elif sched == "dpm2m":
        sch = DPMSolverMultistepScheduler(solver_order=2, **SCHED_KW)
    elif sched == "ddpm_prompts":
        sch = DDPMScheduler(variance_type="fixed_small", clip_sample=False, **SCHED_KW)
        kw = dict(guidance_scale=[7.5, 1.5, 3.0, 5.0, 2.0, 6.5, 4.0][:B], seeds=[100 + b for b in range(B)], prompt_index=[3 * b for b in range(B)])
    else:
        sch, scale = DDIMScheduler(set_alpha_to_one=False, steps_offset=1, clip_sample=False, **SCHED_KW), 1.0
        text = text[B:].contiguous()                                   # no guidance: the conditional rows only
    pipe = LADIFF(denoiser=den, vae=vae, scheduler=sch, guidance_scale=scale, num_inference_timesteps=STEPS, eta=eta, max_it=T,
                  precision=mode, loop=form.split("_")[0])
    noise = syn.init_noise(lens, max_it=T, seed=70 + B).to(DEV)
    L = _lib.lib()
    if form.endswith("look_ahead"):
        _lib.check(L.ladiff_debug_set_loop_thresholds(1, -1))          # look-ahead from one block on: that instantiation runs
    try:
        with torch.no_grad():
            z = pipe._diffusion_reverse(text, lens, init_noise=noise, **kw)
        torch.cuda.synchronize()
    finally:
        L.ladiff_debug_set_loop_thresholds(-1, -1)
    assert pipe.loop_status() == (0, 0)
    assert pipe.last_loop()[0], "the loop did not run as the pipeline kernel"
    return np.ascontiguousarray(z.float().cpu().numpy())


def digest(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def case_key(sched, B, form, mode):
    return f"{sched}_{B}__{form}__{mode}"


@pytest.fixture(scope="module")
def nets():
    return make_nets()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("sched,B", CASES)
def test_step_latents_are_the_parent_librarys_bits(nets, golden, sched, B, form, mode):
    g = golden("step_bits_parent")
    z = loop_latents(nets, sched, B, form, mode)
    key = case_key(sched, B, form, mode)
    idx = g[key + "__idx"].numpy()
    assert np.array_equal(idx, subset_index(B).numpy())
    want = g[key + "__latents"].numpy()
    got = z[:, idx]
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    differ = got.view(np.uint32) != want.view(np.uint32)
    print(f"{key}: {int(differ.sum())} of {differ.size} subset words differ, max |diff| {float(np.abs(got - want).max()):.3e}")
    assert not differ.any(), f"{key}: prompts {sorted(set(idx[np.nonzero(differ)[1]].tolist()))} of the subset differ"
    assert digest(z) == str(g[key + "__sha256"]), f"{key}: the subset agrees but a prompt outside it differs"
