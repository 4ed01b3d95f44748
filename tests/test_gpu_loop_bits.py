"""The loop kernel's latents, bit for bit, against arrays recorded from the library of the commit BEFORE the round-7 work on the
block loops of QKV, OUT and FFN (csrc/systolic.hip).  That work moves and removes instructions on the waves' serial chains and
leaves every product, its order and every rounded value alone, so the tolerance is zero - the same property the tagged-vs-flag
tests of test_gpu_pipeline.py rest on.

Shapes: the headline (128 prompts x 196 frames), c5's mixed lengths (128 prompts of {60, 120, 196} frames) and 256 prompts x 196
frames, each a 50-step DDIM loop with guidance, in both arithmetic modes, on the benchmark's own inputs (bench.Workload draws the
same text embeddings and noise).  The fixture (tests/golden/loop_bits_parent.npz, written by tests/golden/make_golden_loop_bits.py
on the GPU with the parent commit's library) keeps a seeded subset of SUBSET prompts per case and the SHA-256 of the whole
array's bytes: the subset says WHERE latents differ, the digest covers every prompt."""
import hashlib

import numpy as np
import pytest
import torch

from ladiff_amd import LADIFF, DDIMScheduler, LADiffDenoiser, LADiffVae, synthetic as syn
from test_abi import ABL, DEN_KW, VAE_KW

DEV = "cuda:0"
STEPS = 50
SUBSET, SUBSET_SEED = 16, 0
SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False)
CASES = {
    "headline_128x196": lambda: [196] * 128,
    "c5_mixed_128": lambda: syn.mixed_lengths(128),
    "uniform_256x196": lambda: [196] * 256,
}
MODES = ("f16x3", "fp32")


def subset_index(n):
    return torch.randperm(n, generator=torch.Generator().manual_seed(SUBSET_SEED))[:SUBSET].sort().values


def make_nets():
    den = LADiffDenoiser(ABL, **DEN_KW); den.load_state_dict(syn.denoiser_weights(), strict=True)
    vae = LADiffVae(ABL, **VAE_KW); vae.load_state_dict(syn.vae_weights(263), strict=True)
    return den.to(DEV).eval(), vae.to(DEV).eval()


def loop_latents(nets, case, mode):
    """[max_it, B, 256] latents of one 50-step guided DDIM loop through the pipeline kernel, as a numpy float32 array."""
    den, vae = nets
    lens = CASES[case]()
    sch = DDIMScheduler(set_alpha_to_one=False, steps_offset=1, **SCHED_KW)
    pipe = LADIFF(denoiser=den, vae=vae, scheduler=sch, guidance_scale=7.5, num_inference_timesteps=STEPS, eta=0.0, precision=mode)
    text, noise = syn.text_embeddings(len(lens)).to(DEV), syn.init_noise(lens).to(DEV)
    with torch.no_grad():
        z = pipe._diffusion_reverse(text, lens, init_noise=noise)
    torch.cuda.synchronize()
    assert pipe.loop_status() == (0, 0)
    assert pipe.last_loop()[0], "the loop did not run as the pipeline kernel"
    return np.ascontiguousarray(z.float().cpu().numpy())


def digest(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


@pytest.fixture(scope="module")
def nets():
    return make_nets()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_loop_latents_are_the_parent_librarys_bits(nets, golden, case, mode):
    g = golden("loop_bits_parent")
    z = loop_latents(nets, case, mode)
    key = f"{case}__{mode}"
    idx = g[key + "__idx"].numpy()
    assert np.array_equal(idx, subset_index(z.shape[1]).numpy())
    want = g[key + "__latents"].numpy()
    got = z[:, idx]
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    differ = got.view(np.uint32) != want.view(np.uint32)
    print(f"{key}: {int(differ.sum())} of {differ.size} subset words differ, max |diff| {float(np.abs(got - want).max()):.3e}")
    assert not differ.any(), f"{key}: prompts {sorted(set(idx[np.nonzero(differ)[1]].tolist()))} of the subset differ"
    assert digest(z) == str(g[key + "__sha256"]), f"{key}: the subset agrees but a prompt outside it differs"
