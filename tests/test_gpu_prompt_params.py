"""The prompts of one sampling batch as separate requests: a guidance scale and a noise key per prompt (`guidance_scale=`, `seeds=`,
`prompt_index=` of LADIFF.sample; ladiff_diffusion_reverse_prompts).  Against the CPU oracle called once per prompt with that prompt's
scalar, against the scalar call bit for bit where the values coincide, across the block geometries of the pipeline kernel, and - by
counting graph instantiations - that new VALUES in the plan's buffers capture nothing."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ladiff_amd import LADIFF, DDIMScheduler, DDPMScheduler, LADiffDenoiser, LADiffVae, _lib, synthetic as syn
from oracle import ladiff_oracle as orc
from test_abi import ABL, DEN_KW, VAE_KW
from test_gpu_path import FRAME_TOL
from test_gpu_pipeline import SCHED_KW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENS7 = [48, 91, 134, 192, 196, 38, 96]                   # latent counts 1 .. 5 (the formula of test_pipeline_matches_launches at B = 7, T = 5)
SCALES7 = [7.5, 1.5, 3.0, 5.0, 2.0, 6.5, 4.0]
LOOP_TOL = {"f16x3": 2e-4, "fp32": 1e-5}                  # launch-per-stage against the pipeline kernel (tests/test_gpu_pipeline.py)
NOISE_TOL = 4e-6                                          # device generator against numpy (tests/test_noise.py)
_ORACLE = {}


def oracle(key, fn):
    """One CPU oracle run per key for the whole module; nobody writes into what it returns."""
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


@pytest.fixture(scope="module")
def nets():
    den = LADiffDenoiser(ABL, **DEN_KW); den.load_state_dict(syn.denoiser_weights(), strict=True)
    vae = LADiffVae(ABL, **VAE_KW); vae.load_state_dict(syn.vae_weights(263), strict=True)
    return den.to(DEV).eval(), vae.to(DEV).eval()


def make_pipe(nets, loop, precision, sched="ddim", steps=6, T=5, **kw):
    den, vae = nets
    s = (DDIMScheduler(set_alpha_to_one=False, steps_offset=1, **SCHED_KW) if sched == "ddim"
         else DDPMScheduler(variance_type="fixed_small", **SCHED_KW))
    return LADIFF(denoiser=den, vae=vae, scheduler=s, guidance_scale=7.5, num_inference_timesteps=steps, eta=0.0, max_it=T,
                  precision=precision, loop=loop, **kw)


def done(pipe, loop=None):
    assert pipe.loop_status() == (0, 0)
    if loop is not None:
        assert pipe.last_loop()[0] == (loop != "launches")


def sample(pipe, text, lens, loop=None, **kw):
    z, feats = pipe.sample(text.to(DEV), lens, **{k: (v.to(DEV) if torch.is_tensor(v) and v.dim() > 1 else v) for k, v in kw.items()})
    done(pipe, loop)
    return z, feats


def reverse(pipe, text, lens, loop=None, **kw):
    z = pipe._diffusion_reverse(text.to(DEV), lens, **{k: (v.to(DEV) if torch.is_tensor(v) and v.dim() > 1 else v) for k, v in kw.items()})
    done(pipe, loop)
    return z


def maxdiff(a, b):
    return (a.detach().cpu().float() - b.detach().cpu().float()).abs().max().item()


def case7():
    return syn.text_embeddings(7, seed=907), syn.init_noise(LENS7, seed=77)


def oracle_prompt(text, lens, noise, i, scale, steps=6, sched="ddim", step_noise=None, tag="case7"):
    """The oracle on prompt i alone: B = 1, its [uncond, cond] rows, its noise row, its scalar.  scale <= 1: the oracle's no-guidance
    path on the conditional row."""
    B = len(lens)
    rows = text[[i, B + i]] if scale > 1.0 else text[[B + i]]
    return oracle((tag, i, float(scale), steps, sched), lambda: orc.sample_motions(
        syn.denoiser_weights(), syn.vae_weights(263), rows, [lens[i]], noise[i:i + 1], steps, sched, guidance_scale=scale,
        step_noise=step_noise))


# ---------------------------------------------------------------- 1, 2: per-prompt guidance against the oracle
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("loop", ["launches", "pipeline16", "pipeline32"])
def test_per_prompt_guidance_matches_the_oracle_prompt_by_prompt(nets, loop, precision):
    """Seven prompts of latent counts 1 .. 5 at seven scales in one launch.  Every prompt's frames are the oracle's at ITS scale, and -
    for every prompt whose scale is not 7.5 - not the oracle's at 7.5: the oracle's own frames move by 9.2e-2 (6.5 against 7.5) to 3.0
    (1.5 against 7.5), so a kernel that ignored the array or read a neighbour's entry is off by >= 90 gates."""
    text, noise = case7()
    _, feats = sample(make_pipe(nets, loop, precision), text, LENS7, loop, init_noise=noise, guidance_scale=SCALES7)
    _, f75 = oracle(("case7", "all", 7.5), lambda: orc.sample_motions(syn.denoiser_weights(), syn.vae_weights(263), text, LENS7, noise, 6, "ddim"))
    for i, (l, g) in enumerate(zip(LENS7, SCALES7)):
        _, f_o = oracle_prompt(text, LENS7, noise, i, g)
        own, other = maxdiff(feats[i, :l], f_o[0, :l]), maxdiff(feats[i, :l], f75[i, :l])
        print(f"{loop} {precision} prompt {i} scale {g}: |frames - oracle(scale)| = {own:.2e}, |frames - oracle(7.5)| = {other:.2e}")
        assert own < FRAME_TOL
        assert other < FRAME_TOL if g == 7.5 else other >= FRAME_TOL


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("loop", ["launches", "pipeline16", "pipeline32"])
def test_scale_one_is_the_conditional_prediction(nets, loop, precision):
    """A per-prompt 1.0 is simply evaluated - eps_u + 1.0 (eps_c - eps_u) - and lands on the oracle's no-guidance path on the
    conditional row (oracle, guided formula at 1 + 1e-7 against that path: 7.0e-6 on the frames)."""
    text, noise = case7()
    scales = list(SCALES7)
    scales[3] = 1.0
    _, feats = sample(make_pipe(nets, loop, precision), text, LENS7, loop, init_noise=noise, guidance_scale=scales)
    for i in (3, 4):                                                # the prompt at 1.0 and a neighbour in its block
        _, f_o = oracle_prompt(text, LENS7, noise, i, scales[i])
        err = maxdiff(feats[i, :LENS7[i]], f_o[0, :LENS7[i]])
        print(f"{loop} {precision} prompt {i} scale {scales[i]}: |frames - oracle| = {err:.2e}")
        assert err < FRAME_TOL


# ---------------------------------------------------------------- 3: block geometry
_LAUNCHES = {}


@pytest.mark.parametrize("loop", ["pipeline16", "pipeline32", "pipeline"])
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("B,T", [(1, 5), (3, 5), (7, 5), (43, 5), (9, 2), (5, 8)])
def test_every_block_geometry_picks_the_pair_s_own_scale(nets, loop, precision, B, T):
    """16-row blocks hold several prompts of different latent counts, 32-row blocks both branches of up to three prompts: each
    (prompt, latent) pair must be guided by its own prompt's scale, as the launch-per-stage loop's tail launch does row by row."""
    lens = [max(1, min(196, 48 * ((i % T) + 1) - 5 * (i % 3))) for i in range(B)]
    scales = [1.5 + (b % 5) for b in range(B)]
    text = syn.text_embeddings(B, seed=900 + B)
    noise = torch.randn(B, T, 256, generator=torch.Generator().manual_seed(B * 10 + T))
    if (precision, B, T) not in _LAUNCHES:
        _LAUNCHES[(precision, B, T)] = reverse(make_pipe(nets, "launches", precision, T=T), text, lens, "launches", init_noise=noise,
                                               guidance_scale=scales)
    za = _LAUNCHES[(precision, B, T)]
    zb = reverse(make_pipe(nets, loop, precision, T=T), text, lens, loop, init_noise=noise, guidance_scale=scales)
    scale = max(1.0, za.abs().max().item())
    assert torch.isfinite(zb).all()
    assert maxdiff(za, zb) < LOOP_TOL[precision] * scale
    for i, l in enumerate(lens):                                    # rows past a motion's latent count: exact zeros
        c = -(-l // 48)
        if c < T:
            assert zb[c:, i].abs().max().item() == 0 and za[c:, i].abs().max().item() == 0


# ---------------------------------------------------------------- 4: nothing changes for the scalar call, bit for bit
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("loop", ["launches", "pipeline"])
def test_an_array_of_the_scalar_gives_the_scalar_call_s_bits(nets, loop, precision):
    text, noise = case7()
    pipe = make_pipe(nets, loop, precision)
    z_scalar = reverse(pipe, text, LENS7, loop, init_noise=noise)
    z_array = reverse(pipe, text, LENS7, loop, init_noise=noise, guidance_scale=[7.5] * 7)
    z_number = reverse(pipe, text, LENS7, loop, init_noise=noise, guidance_scale=7.5)
    assert torch.equal(z_array, z_scalar) and torch.equal(z_number, z_scalar)
    assert not torch.equal(reverse(pipe, text, LENS7, loop, init_noise=noise, guidance_scale=SCALES7), z_scalar)


@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("loop", ["launches", "pipeline"])
def test_per_prompt_keys_that_restate_the_call_seed_give_its_bits(nets, loop, first):
    """seeds = [S] * B with prompt_index = first_prompt + b is the scalar generator's (seed, global prompt) pair by pair."""
    text, noise = case7()
    S = 0xC0FFEE1234
    pipe = make_pipe(nets, loop, "f16x3", sched="ddpm", steps=5)
    pipe.noise_first_prompt = first
    z_seed = reverse(pipe, text, LENS7, loop, init_noise=noise, noise_seed=S)
    z_keys = reverse(pipe, text, LENS7, loop, init_noise=noise, seeds=[S] * 7, prompt_index=[first + b for b in range(7)])
    assert torch.isfinite(z_seed).all() and torch.equal(z_keys, z_seed)
    assert not torch.equal(reverse(pipe, text, LENS7, loop, init_noise=noise, seeds=[S] * 7, prompt_index=[first + b + 1 for b in range(7)]), z_seed)


# ---------------------------------------------------------------- 5: per-prompt seeds against the oracle
SEEDS3, INDEX3, LENS3 = [11, 2 ** 40 + 5, 11], [0, 3, 1], [196, 60, 130]


def oracle_noise3():
    """Per prompt: (initial noise [1,T,256] at schedule position -1, step noise [5,1,T,256]) of the numpy generator."""
    return oracle("noise3", lambda: [(torch.from_numpy(orc.device_noise(s, ix, 2 ** 32 - 1, 1, 1, 5))[0],
                                      torch.from_numpy(orc.device_noise(s, ix, 0, 5, 1, 5))) for s, ix in zip(SEEDS3, INDEX3)])


def test_per_prompt_noise_tensor_matches_the_numpy_generator():
    got = LADIFF.noise_tensor(None, 6, 3, 5, first_step=-1, device=DEV, seeds=SEEDS3, prompt_index=INDEX3).cpu()
    for b, (init, steps) in enumerate(oracle_noise3()):
        e0, e1 = maxdiff(got[0, b], init[0]), maxdiff(got[1:, b], steps[:, 0])
        print(f"prompt {b} (seed {SEEDS3[b]:#x}, index {INDEX3[b]}): position -1 {e0:.2e}, positions 0..4 {e1:.2e}")
        assert e0 < NOISE_TOL and e1 < NOISE_TOL
    assert maxdiff(got[:, 0], got[:, 2]) > 1.0                      # same seed, another index: other noise
    assert maxdiff(got[0], got[1]) > 1.0                            # position -1 is not position 0
    no_index = LADIFF.noise_tensor(None, 1, 3, 5, first_step=-1, device=DEV, seeds=SEEDS3).cpu()
    assert torch.equal(no_index[0, 0], got[0, 0]) and torch.equal(no_index[0, 0], no_index[0, 2])      # no index: word 1 = 0
    # the scalar fill at the same (seed, prompt): the same bits
    assert torch.equal(LADIFF.noise_tensor(11, 5, 1, 5, first_prompt=1, device=DEV).cpu()[:, 0], got[1:, 2])


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("loop", ["launches", "pipeline"])
def test_per_prompt_seeds_match_the_oracle_fed_the_numpy_noise(nets, loop, precision):
    """DDPM, 5 steps, no init_noise: initial and step noise both come from each prompt's (seed, index) on the device."""
    text = syn.text_embeddings(3, seed=43)
    torch.manual_seed(99)
    state = torch.get_rng_state()
    _, feats = sample(make_pipe(nets, loop, precision, sched="ddpm", steps=5), text, LENS3, loop, seeds=SEEDS3, prompt_index=INDEX3)
    assert torch.equal(torch.get_rng_state(), state)                # torch's generator was not touched
    frames = []
    for i, (init, steps) in enumerate(oracle_noise3()):
        _, f_o = oracle(("seeds3", i), lambda: orc.sample_motions(syn.denoiser_weights(), syn.vae_weights(263), text[[i, 3 + i]], [LENS3[i]],
                                                                  init, 5, "ddpm", step_noise=steps))
        assert torch.isfinite(f_o).all()
        err = maxdiff(feats[i, :LENS3[i]], f_o[0])
        print(f"{loop} {precision} prompt {i}: |frames - oracle| = {err:.2e} (oracle max {f_o.abs().max().item():.2f})")
        assert err < FRAME_TOL
        frames.append(f_o[0])
    assert maxdiff(frames[0][:60], frames[2][:60]) > FRAME_TOL     # the two prompts with seed 11 differ (index 0 against 1) ...
    text_same = torch.cat([text[[0, 0, 0]], text[[3, 3, 3]]])       # ... also with the same text and length
    z = reverse(make_pipe(nets, loop, precision, sched="ddpm", steps=5), text_same, [196] * 3, loop, seeds=SEEDS3, prompt_index=INDEX3)
    assert maxdiff(z[:, 0], z[:, 2]) > 1e-2


# ---------------------------------------------------------------- 6: a request does not depend on its batch
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("loop", ["launches", "pipeline16", "pipeline32"])
def test_a_request_gives_the_same_motion_alone_and_among_others(nets, loop, precision):
    """Prompt 4 of the seven with (seed, index, scale) of its own: alone, and third of five other texts and lengths.  (Bit equality
    is not asserted: DESIGN.md 8e records where it was seen.)"""
    text, _ = case7()
    other = syn.text_embeddings(5, seed=31)
    seed, index, g = 0xABCDEF0123, 17, 2.0
    alone = reverse(make_pipe(nets, loop, precision, sched="ddpm", steps=5), text[[4, 11]], [196], loop, seeds=[seed], prompt_index=[index],
                    guidance_scale=[g])
    mixed_text = other.clone()
    mixed_text[2], mixed_text[7] = text[4], text[11]
    among = reverse(make_pipe(nets, loop, precision, sched="ddpm", steps=5), mixed_text, [60, 150, 196, 30, 100], loop,
                    seeds=[1, 2, seed, 4, 5], prompt_index=[0, 1, index, 3, 4], guidance_scale=[7.5, 3.0, g, 5.0, 1.5])
    err, scale = maxdiff(alone[:, 0], among[:, 2]), max(1.0, alone.abs().max().item())
    print(f"{loop} {precision}: alone against third of five: {err:.2e} (scale {scale:.2f}), bit-equal: {torch.equal(alone[:, 0], among[:, 2])}")
    assert torch.isfinite(alone).all() and err < LOOP_TOL[precision] * scale


# ---------------------------------------------------------------- 7: the capture key holds pointers, not values
def counted(fn):
    L = _lib.lib()
    before = L.ladiff_debug_graph_instantiations()
    out = fn()
    torch.cuda.synchronize()
    return out, L.ladiff_debug_graph_instantiations() - before


@pytest.mark.parametrize("loop,per_capture", [("launches", 2), ("pipeline", 1)])
def test_new_values_replay_the_graphs_and_change_the_result(nets, loop, per_capture):
    text, noise = case7()
    pipe = make_pipe(nets, loop, "f16x3", sched="ddpm", steps=3)
    scalar = lambda: reverse(pipe, text, LENS7, loop, init_noise=noise, noise_seed=5)
    arrays = lambda g, s: (lambda: reverse(pipe, text, LENS7, loop, guidance_scale=g, seeds=s, prompt_index=list(range(7))))
    z0, n = counted(scalar)
    assert n == per_capture
    z1, n = counted(arrays(SCALES7, [3] * 7))
    print(f"{loop}: first call with arrays: +{n}")
    assert n == per_capture                                         # three pointers and the draw flag joined the key
    z2, n = counted(arrays(SCALES7[::-1], [3] * 7))
    print(f"{loop}: other scales: +{n}")
    assert n == 0 and not torch.equal(z2, z1)
    z3, n = counted(arrays(SCALES7[::-1], [4] * 7))
    print(f"{loop}: other seeds: +{n}")
    assert n == 0 and not torch.equal(z3, z2)
    z4, n = counted(arrays(SCALES7, [3] * 7))
    assert n == 0 and torch.equal(z4, z1)                           # the first values again: the first result
    z5, n = counted(scalar)
    print(f"{loop}: without arrays again: +{n}")
    assert n == per_capture and torch.equal(z5, z0)


# ---------------------------------------------------------------- 8: the other paths
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_chunked_batch_slices_the_arrays(nets, precision):
    text, _ = case7()
    kw = dict(guidance_scale=SCALES7, seeds=[100 + b for b in range(7)], prompt_index=[3 * b for b in range(7)])
    whole = reverse(make_pipe(nets, "pipeline", precision, sched="ddpm", steps=5), text, LENS7, "pipeline", **kw)
    chunked_pipe = make_pipe(nets, "pipeline", precision, sched="ddpm", steps=5, max_prompts_per_launch=4)
    chunked_pipe.noise_first_prompt = 9                             # shifts the scalar generator's prompts, not a caller's index
    chunks = reverse(chunked_pipe, text, LENS7, "pipeline", **kw)
    assert len(chunked_pipe._last) == 2
    assert maxdiff(whole, chunks) < LOOP_TOL[precision] * max(1.0, whole.abs().max().item())


def test_many_text_tokens_take_the_arrays_through_the_tail_launch(nets):
    """n_text = 4 runs launch per stage whatever the loop form asked for; the guidance array reaches its tail launch."""
    B, lens, scales = 3, [196, 60, 130], [2.0, 7.5, 4.5]
    gen = torch.Generator().manual_seed(404)
    text, noise = torch.randn(2 * B, 4, 768, generator=gen), syn.init_noise(lens, seed=405)
    _, feats = sample(make_pipe(nets, "launches", "fp32"), text, lens, "launches", init_noise=noise, guidance_scale=scales)
    for i in range(B):
        _, f_o = oracle_prompt(text, lens, noise, i, scales[i], tag="n_text4")
        err = maxdiff(feats[i, :lens[i]], f_o[0, :lens[i]])
        print(f"n_text 4 prompt {i} scale {scales[i]}: |frames - oracle| = {err:.2e}")
        assert err < FRAME_TOL


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_plain_launches_without_a_sampler_take_the_same_arguments(nets, precision):
    text, _ = case7()
    kw = dict(guidance_scale=SCALES7, seeds=[100 + b for b in range(7)], prompt_index=[3 * b for b in range(7)])
    with_sampler = reverse(make_pipe(nets, "launches", precision, sched="ddpm", steps=5), text, LENS7, "launches", **kw)
    plain_pipe = make_pipe(nets, "launches", precision, sched="ddpm", steps=5, use_graph=False)
    plain = plain_pipe._diffusion_reverse(text.to(DEV), LENS7, **kw)
    assert plain_pipe.loop_status() == (0, 0)
    assert all(p["step_noise"] is None and p["sampler"] is None for p in plain_pipe._plans.values())      # no [n,B,T,256] tensor was made
    assert maxdiff(with_sampler, plain) < LOOP_TOL[precision] * max(1.0, with_sampler.abs().max().item())


def test_forward_reads_the_two_optional_batch_keys(nets):
    den, vae = nets
    lens, scales, seeds = [196, 60, 130], [2.0, 7.5, 4.5], [5, 6, 7]
    enc_out = torch.randn(6, 1, 768, generator=torch.Generator().manual_seed(97)).to(DEV)
    dm = SimpleNamespace(feats2joints=None, hparams=SimpleNamespace(mean=np.zeros(263, dtype=np.float32), std=np.ones(263, dtype=np.float32)),
                         njoints=22)
    model = LADIFF(None, dm, denoiser=den, vae=vae, text_encoder=lambda texts: enc_out, guidance_scale=7.5, num_inference_timesteps=5,
                   scheduler=DDPMScheduler(variance_type="fixed_small", **SCHED_KW))
    joints = model.forward({"text": ["a", "b", "c"], "length": lens, "guidance_scale": scales, "seed": seeds})
    assert model.loop_status() == (0, 0)
    _, feats = model.sample(enc_out, lens, guidance_scale=scales, seeds=seeds)
    assert model.loop_status() == (0, 0)
    want = model.feats2joints_device(feats).cpu()
    for i, l in enumerate(lens):
        assert joints[i].shape[0] == l and torch.equal(joints[i], want[i, :l])
    other = model.forward({"text": ["a", "b", "c"], "length": lens, "guidance_scale": scales, "seed": [5, 6, 8]})
    assert torch.equal(other[0], joints[0]) and not torch.equal(other[2], joints[2])      # only the request whose seed changed moves
