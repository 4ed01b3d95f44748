"""Motion editing on the GPU (a loop from a source motion): the prologue kernel against numpy, the freeze and the start
at position 0 bit for bit, every prompt against the CPU oracle restarted at its own start (tests/edit_ref.py), independence of the
batch, the block geometries of the pipeline kernel, windows, graph replays, `LADIFF.edit` end to end and the loop without a sampler.
T = 5, 6 steps; 7 prompts of latent counts 1 .. 5 (two tail units: no prefetch) and 43 prompts (more than NTAIL units: prefetch, m1
travels in Pay), the shapes of tests/test_gpu_step_bits.py and tests/test_gpu_prompt_params.py."""
from contextlib import contextmanager
from types import SimpleNamespace

import pytest
import torch

from ladiff_amd import LADIFF, DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, LADiffDenoiser, LADiffVae, _lib, synthetic as syn
from oracle import ladiff_oracle as orc
import edit_ref
from test_abi import ABL, DEN_KW, VAE_KW
from test_gpu_path import FRAME_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
LENS7 = [48, 91, 134, 192, 196, 38, 96]                   # latent counts 1 .. 5
SCALES7 = [7.5, 1.5, 3.0, 5.0, 2.0, 6.5, 4.0]
STARTS7 = [0, 1, 2, 3, 4, 5, 2]
SEEDS7, INDEX7 = [100 + b for b in range(7)], [3 * b for b in range(7)]
LOOP_TOL = {"f16x3": 2e-4, "fp32": 1e-5}                  # launch-per-stage against the pipeline kernel (tests/test_gpu_pipeline.py)
NOISE_TOL = 4e-6                                          # device generator against numpy (tests/test_noise.py)
FORMS = ["launches", "pipeline16", "pipeline16_look_ahead", "pipeline32"]
MODES = ["fp32", "f16x3"]
SCHEDS = ["ddim", "ddpm", "dpm"]
POSITIONS = {"ddim": 6, "ddpm": 7, "dpm": 6}              # DDPMScheduler.set_timesteps(6) yields arange(0, 1000, 166): seven positions
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


def scheduler(sched):
    if sched == "ddim":
        return DDIMScheduler(set_alpha_to_one=False, steps_offset=1, clip_sample=False, **SCHED_KW)
    if sched == "ddpm":
        return DDPMScheduler(variance_type="fixed_small", clip_sample=False, **SCHED_KW)
    return DPMSolverMultistepScheduler(solver_order=2, **SCHED_KW)


def make_pipe(nets, form, precision, sched="ddim", steps=6, T=5, **kw):
    den, vae = nets
    return LADIFF(denoiser=den, vae=vae, scheduler=scheduler(sched), guidance_scale=7.5, num_inference_timesteps=steps, eta=0.0, max_it=T,
                  precision=precision, loop=form.split("_")[0], **kw)


@contextmanager
def loop_form(form):
    """pipeline16_look_ahead: 16-row blocks with the look-ahead instantiation forced in (as tests/test_gpu_step_bits.py does)."""
    L = _lib.lib()
    if form.endswith("look_ahead"):
        _lib.check(L.ladiff_debug_set_loop_thresholds(1, -1))
    try:
        yield
    finally:
        L.ladiff_debug_set_loop_thresholds(-1, -1)


def reverse(pipe, form, text, lens, **kw):
    with loop_form(form), torch.no_grad():
        z = pipe._diffusion_reverse(text.to(DEV), lens, **{k: (v.to(DEV) if torch.is_tensor(v) and v.dim() > 1 else v) for k, v in kw.items()})
        torch.cuda.synchronize()
    assert pipe.loop_status() == (0, 0)
    assert pipe.last_loop()[0] == (form != "launches")
    return z


def maxdiff(a, b):
    return (a.detach().cpu().float() - b.detach().cpu().float()).abs().max().item()


def case7():
    """texts, initial noise [7,5,256] and source latents [5,7,256] of the seven prompts (fixed seeds: the oracle's separation between
    neighbouring starts, asserted in test 4, was measured on the CPU with exactly these)."""
    return syn.text_embeddings(7, seed=907), syn.init_noise(LENS7, seed=77), torch.randn(5, 7, 256, generator=torch.Generator().manual_seed(2024))


def noise_args(sched, noise, B=7):
    """How a schedule gets its noise here: DDIM and the multistep rule take an init_noise tensor, DDPM draws everything from the
    per-prompt generator (initial noise at position -1 included)."""
    return dict(seeds=SEEDS7[:B], prompt_index=INDEX7[:B]) if sched == "ddpm" else dict(init_noise=noise)


def poison_x0_prev(pipe):
    for plan in pipe._plans.values():
        if "x0_prev" in plan:
            plan["x0_prev"].fill_(float("nan"))


def init_from(z0, noise, coef, starts, first_step, counts, seeds=None, index=None):
    """ladiff_init_latents_from on device tensors -> latents [B,T,256]."""
    T, B = z0.shape[0], z0.shape[1]
    out = torch.full((B, T, 256), float("nan"), dtype=torch.float32, device=DEV)
    d = lambda v, dt: None if v is None else torch.tensor(v, dtype=dt, device=DEV)
    cd, sd, id_, st = d(counts, torch.int32), d(seeds, torch.int64), d(index, torch.int32), d(starts, torch.int32)
    p = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.lib().ladiff_init_latents_from(_lib.ptr(z0), None if noise is None else _lib.ptr(noise), p(sd), p(id_), p(cd), _lib.ptr(coef),
                                                   p(st), first_step, _lib.ptr(out), B, T, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------- 1: the prologue kernel against numpy
def test_prologue_kernel_matches_numpy():
    """latents = valid (alpha(s_b) z0 + sigma(s_b) noise) with the noise of each prompt's own (seed, index) at position -1; the gate is
    the generator's own (device ln / cos / sin against numpy's, NOISE_TOL) scaled by the result's magnitude.  Rows past the count: 0."""
    _, _, z0 = case7()
    sch = scheduler("ddim")
    sch.set_timesteps(6)
    coef = sch.coef_table(0.0)
    counts = [1, 2, 3, 4, 5, 1, 2]
    got = init_from(z0.to(DEV), None, coef.to(DEV), STARTS7, 0, counts, SEEDS7, INDEX7).cpu()
    worst = 0.0
    for b in range(7):
        nz = torch.from_numpy(orc.device_noise(SEEDS7[b], INDEX7[b], 2 ** 32 - 1, 1, 1, 5))[0, 0].double()
        want = float(coef[STARTS7[b], 0]) * z0[:, b].double() + float(coef[STARTS7[b], 1]) * nz
        c = counts[b]
        err, scale = (got[b, :c].double() - want[:c]).abs().max().item(), max(1.0, want[:c].abs().max().item())
        print(f"prompt {b} start {STARTS7[b]}: |latents - numpy| = {err:.2e} (scale {scale:.2f})")
        assert err < NOISE_TOL * scale
        assert c == 5 or got[b, c:].abs().max().item() == 0
        worst = max(worst, err)
    # the noise tensor form and NULL starts: every prompt at first_step
    noise = torch.randn(7, 5, 256, generator=torch.Generator().manual_seed(5))
    got = init_from(z0.to(DEV), noise.to(DEV), coef.to(DEV), None, 3, None).cpu()
    want = float(coef[3, 0]) * z0.permute(1, 0, 2).double() + float(coef[3, 1]) * noise.double()
    assert (got.double() - want).abs().max().item() < 1e-6 * max(1.0, want.abs().max().item())


# ---------------------------------------------------------------- 2: the freeze is exact
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("sched", SCHEDS)
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("form", FORMS)
def test_frozen_positions_leave_no_trace(nets, form, precision, sched, k):
    """starts = [k] * B with first_step = 0 runs positions 0 .. k - 1 with every prompt frozen, then the loop; first_step = k without an
    array never runs them.  Same bits.  Multistep form: x0_prev holds NaN on entry, so a read of m1 at s_b would show."""
    text, noise, z0 = case7()
    pipe = make_pipe(nets, form, precision, sched)
    kw = dict(source_latents=z0, **noise_args(sched, noise))
    poison_x0_prev(pipe)
    za = reverse(pipe, form, text, LENS7, start_steps=[k] * 7, first_step=0, **kw)
    poison_x0_prev(pipe)
    zb = reverse(pipe, form, text, LENS7, first_step=k, **kw)
    assert torch.isfinite(za).all() and torch.isfinite(zb).all()
    assert torch.equal(za, zb)
    assert not torch.equal(za, reverse(pipe, form, text, LENS7, first_step=k - 1, **kw))       # the start matters at all


# ---------------------------------------------------------------- 3: start 0 is today's loop
@pytest.mark.parametrize("sched", SCHEDS)
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("form", FORMS)
def test_start_zero_is_the_loop_from_noise(nets, form, precision, sched):
    """z0 with every start at 0 = the loop without z0 fed the prologue kernel's output as init_noise (init_noise_sigma is 1)."""
    text, noise, z0 = case7()
    pipe = make_pipe(nets, form, precision, sched)
    assert pipe.scheduler.init_noise_sigma == 1.0
    z_edit = reverse(pipe, form, text, LENS7, source_latents=z0, start_steps=[0] * 7, **noise_args(sched, noise))
    plan = pipe._plan
    gen = sched == "ddpm"
    lat = init_from(z0.to(DEV), None if gen else noise.to(DEV), plan["coef"], [0] * 7, 0, None, SEEDS7 if gen else None, INDEX7 if gen else None)
    z_plain = reverse(pipe, form, text, LENS7, init_noise=lat, **({"seeds": SEEDS7, "prompt_index": INDEX7} if gen else {}))
    assert torch.isfinite(z_edit).all() and torch.equal(z_edit, z_plain)


# ---------------------------------------------------------------- 4: against the oracle, prompt by prompt
def oracle_edit(sched, i, start, text, noise, z0):
    def run():
        if sched == "ddpm":
            init, steps = edit_ref.generator_noise(SEEDS7[i], INDEX7[i], POSITIONS[sched], 5)
        else:
            init, steps = noise[i], None
        return edit_ref.edit_prompt(text[[i, 7 + i]], LENS7[i], z0[:, i], init, start, 6, sched, SCALES7[i], steps)[1]
    return oracle((sched, i, start), run)


@pytest.mark.parametrize("sched", SCHEDS)
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("form", FORMS)
def test_every_prompt_matches_the_oracle_restarted_at_its_own_start(nets, form, precision, sched):
    """Seven prompts, starts 0 1 2 3 4 5 2, a scale (and under DDPM a noise key) per prompt, one launch.  The oracle's own frames at s_b
    and at the neighbouring start differ by 0.41 .. 3.9 (measured on the CPU for the three schedules; asserted >= 10 gates below), so an
    off-by-one start cannot pass.  Measured |frames - oracle| per loop form and mode: DESIGN.md 8h."""
    text, noise, z0 = case7()
    for i, s in enumerate(STARTS7):
        near = s + 1 if s + 1 < 6 else s - 1
        sep = maxdiff(oracle_edit(sched, i, s, text, noise, z0), oracle_edit(sched, i, near, text, noise, z0))
        assert sep >= 10 * FRAME_TOL, (sched, i, sep)
    pipe = make_pipe(nets, form, precision, sched)
    with loop_form(form):
        _, feats = pipe.sample(text.to(DEV), LENS7, guidance_scale=SCALES7, source_latents=z0.to(DEV), start_steps=STARTS7,
                               **{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in noise_args(sched, noise).items()})
    assert pipe.loop_status() == (0, 0) and pipe.last_loop()[0] == (form != "launches")
    worst = 0.0
    for i, (l, s) in enumerate(zip(LENS7, STARTS7)):
        err = maxdiff(feats[i, :l], oracle_edit(sched, i, s, text, noise, z0)[0, :l])
        worst = max(worst, err)
        print(f"{sched} {form} {precision} prompt {i} start {s}: |frames - oracle| = {err:.2e}")
        assert err < FRAME_TOL
    print(f"{sched} {form} {precision}: worst |frames - oracle| = {worst:.2e}")


# ---------------------------------------------------------------- 5: a request does not depend on its batch
@pytest.mark.parametrize("sched", ["ddpm", "dpm"])
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("form", ["launches", "pipeline16", "pipeline32"])
def test_a_request_gives_the_same_motion_alone_and_among_others(nets, form, precision, sched):
    """Prompt 4 of the seven, start 3: alone (first_step = 3) and third of five with other texts, lengths and starts (first_step = 0).
    Bit for bit in both pipeline geometries; LOOP_TOL launch per stage (DESIGN.md 8e records why)."""
    text, noise, z0 = case7()
    other = syn.text_embeddings(5, seed=31)
    z_other = torch.randn(5, 5, 256, generator=torch.Generator().manual_seed(32))
    z_other[:, 2] = z0[:, 4]
    n_other = torch.randn(5, 5, 256, generator=torch.Generator().manual_seed(33))
    n_other[2] = noise[4]
    seed, index, g = 0xABCDEF0123, 17, 2.0
    own = lambda nz: dict(seeds=[seed], prompt_index=[index]) if sched == "ddpm" else dict(init_noise=nz)
    alone = reverse(make_pipe(nets, form, precision, sched), form, text[[4, 11]], [196], guidance_scale=[g], source_latents=z0[:, 4:5],
                    start_steps=[3], **own(noise[4:5]))
    mixed_text = other.clone()
    mixed_text[2], mixed_text[7] = text[4], text[11]
    many = dict(seeds=[1, 2, seed, 4, 5], prompt_index=[0, 1, index, 3, 4]) if sched == "ddpm" else dict(init_noise=n_other)
    among = reverse(make_pipe(nets, form, precision, sched), form, mixed_text, [60, 150, 196, 30, 100], guidance_scale=[7.5, 3.0, g, 5.0, 1.5],
                    source_latents=z_other, start_steps=[0, 5, 3, 1, 4], **many)
    err, scale = maxdiff(alone[:, 0], among[:, 2]), max(1.0, alone.abs().max().item())
    print(f"{sched} {form} {precision}: alone against third of five: {err:.2e} (scale {scale:.2f})")
    assert torch.isfinite(alone).all()
    if form == "launches":
        assert err < LOOP_TOL[precision] * scale
    else:
        assert torch.equal(alone[:, 0], among[:, 2])


# ---------------------------------------------------------------- 6: block geometries
_LAUNCHES = {}


@pytest.mark.parametrize("form", ["pipeline16", "pipeline32", "pipeline"])
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("B,T", [(1, 5), (3, 5), (7, 5), (43, 5), (9, 2), (5, 8)])
def test_every_block_geometry_picks_the_pair_s_own_start(nets, form, precision, B, T):
    """Starts b % 6 under the multistep rule (frozen pairs, first-order pairs and second-order pairs side by side in one block): each
    (prompt, latent) pair must be gated by its own prompt's start, as the launch-per-stage loop's tail launch does row by row."""
    lens = [max(1, min(196, 48 * ((i % T) + 1) - 5 * (i % 3))) for i in range(B)]
    starts = [b % 6 for b in range(B)]
    text = syn.text_embeddings(B, seed=900 + B)
    noise = torch.randn(B, T, 256, generator=torch.Generator().manual_seed(B * 10 + T))
    z0 = torch.randn(T, B, 256, generator=torch.Generator().manual_seed(B * 10 + T + 1))
    kw = dict(init_noise=noise, source_latents=z0, start_steps=starts)
    if (precision, B, T) not in _LAUNCHES:
        _LAUNCHES[(precision, B, T)] = reverse(make_pipe(nets, "launches", precision, "dpm", T=T), "launches", text, lens, **kw)
    za = _LAUNCHES[(precision, B, T)]
    zb = reverse(make_pipe(nets, form, precision, "dpm", T=T), form, text, lens, **kw)
    scale = max(1.0, za.abs().max().item())
    assert torch.isfinite(zb).all()
    assert maxdiff(za, zb) < LOOP_TOL[precision] * scale
    for i, l in enumerate(lens):                                    # rows past a motion's latent count: exact zeros
        c = -(-l // 48)
        if c < T:
            assert zb[c:, i].abs().max().item() == 0 and za[c:, i].abs().max().item() == 0


# ---------------------------------------------------------------- 7: windows
def step_counter(pipe):
    return int(pipe._plan["ws"][:1].view(torch.int32).item())     # word 0 of the workspace (csrc/workspace.h, carve_reverse)


@pytest.mark.parametrize("first", [None, 40])
@pytest.mark.parametrize("precision", MODES)
def test_starts_on_both_sides_of_a_window_boundary(nets, precision, first):
    """66 steps run as two windows of 33.  first = None: starts 20 and 40 alternate, the first window is partial (positions 20 .. 32).
    first = 40: every prompt starts inside the SECOND window, which is then the only launch.  Pipeline against plain launches within the
    windowed gate of test_gpu_dpm_solver.py; the launch-per-stage loop's step counter ends at n, so n - first_step denoiser steps ran
    and none at a position >= n; the pipeline's prologue leaves it at first_step."""
    n = 66
    text, noise, z0 = case7()
    starts = [20, 40, 20, 40, 40, 20, 40] if first is None else [40] * 7
    lo = min(starts)
    kw = dict(init_noise=noise, source_latents=z0, start_steps=starts)
    pipe = make_pipe(nets, "pipeline", precision, "dpm", steps=n)
    pipe.window_ms(enable=True)
    zp = reverse(pipe, "pipeline", text, LENS7, **kw)
    assert pipe.window_ms()[1] == (2 if lo < 33 else 1)
    assert step_counter(pipe) == lo
    graphs = make_pipe(nets, "launches", precision, "dpm", steps=n)
    zg = reverse(graphs, "launches", text, LENS7, **kw)
    assert step_counter(graphs) == n
    plain = make_pipe(nets, "launches", precision, "dpm", steps=n, use_graph=False)
    with torch.no_grad():
        zl = plain._diffusion_reverse(text.to(DEV), LENS7, **{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()})
    torch.cuda.synchronize()
    assert plain.loop_status() == (0, 0) and step_counter(plain) == n
    scale = max(1.0, zl.abs().max().item())
    print(f"{precision} first {lo}: pipeline against plain launches {maxdiff(zp, zl):.2e}, step graphs {maxdiff(zg, zl):.2e} (scale {scale:.2f})")
    assert torch.isfinite(zp).all() and maxdiff(zp, zl) < LOOP_TOL[precision] * scale
    assert maxdiff(zg, zl) < LOOP_TOL[precision] * scale


# ---------------------------------------------------------------- 8: replays
def counted(fn):
    L = _lib.lib()
    before = L.ladiff_debug_graph_instantiations()
    out = fn()
    torch.cuda.synchronize()
    return out, L.ladiff_debug_graph_instantiations() - before


@pytest.mark.parametrize("form,per_capture", [("launches", 2), ("pipeline", 1)])
def test_new_starts_replay_the_graphs_and_change_the_result(nets, form, per_capture):
    text, noise, z0 = case7()
    pipe = make_pipe(nets, form, "f16x3", "dpm")
    plain = lambda: reverse(pipe, form, text, LENS7, init_noise=noise)
    edit = lambda src, starts, first=None: (lambda: reverse(pipe, form, text, LENS7, init_noise=noise, source_latents=src, start_steps=starts,
                                                            first_step=first))
    z_plain, n = counted(plain)
    assert n == per_capture
    z1, n = counted(edit(z0, STARTS7))
    print(f"{form}: first call with z0: +{n}")
    assert n == per_capture
    z2, n = counted(edit(z0, [2, 2, 3, 3, 2, 5, 2], first=0 if form == "launches" else None))
    print(f"{form}: other starts: +{n}")
    assert n == 0 and not torch.equal(z2, z1)
    if form == "pipeline":                                            # another first_step is a launch argument of the pipeline kernel
        z3, n = counted(edit(z0, [2, 2, 3, 3, 2, 5, 2], first=0))
        print(f"{form}: another first_step: +{n}")
        assert n == 0 and torch.equal(z3, z2)
    z4, n = counted(edit(-z0, STARTS7))
    print(f"{form}: other source latents in the same buffer: +{n}")
    assert n == 0 and not torch.equal(z4, z1)
    z5, n = counted(edit(z0, STARTS7))
    assert n == 0 and torch.equal(z5, z1)
    z6, n = counted(plain)
    print(f"{form}: without z0 again: +{n}")
    assert n == per_capture and torch.equal(z6, z_plain)


# ---------------------------------------------------------------- 9: LADIFF.edit end to end
LENS3 = [196, 60, 130]
JOINT_STD = 0.1           # the datamodule's feature std of the end-to-end tests, see test_edit_from_a_motion_matches_the_oracle_chain


def edit_model(nets, enc_out, sched="ddim", **kw):
    den, vae = nets
    mean, std = torch.zeros(263), torch.full((263,), JOINT_STD)
    dm = SimpleNamespace(feats2joints=None, hparams=SimpleNamespace(mean=mean.numpy(), std=std.numpy()), njoints=22)
    return LADIFF(None, dm, denoiser=den, vae=vae, text_encoder=lambda texts: enc_out.to(DEV), guidance_scale=7.5, num_inference_timesteps=6,
                  scheduler=scheduler(sched), **kw)


@pytest.mark.parametrize("precision", MODES)
def test_edit_from_a_motion_matches_the_oracle_chain(nets, precision):
    """batch["motion"] -> vae.encode (its sample, with the eps given) -> prologue -> loop -> decode -> joints, a strength per prompt,
    against oracle.vae_encode with the same eps -> edit_ref -> oracle.feats2joints, at the project's one gate on the joints.
    The datamodule's statistics are mean 0, std 0.1: feats2joints integrates the root's yaw and planar velocity over the frames, and on
    the oracle ALONE a 1e-5 perturbation of unit-variance frames (100 times inside the frame gate) moves the joints of a 196-frame
    motion by 6.1e-3 under std 1 (yaw velocity ~1 rad per frame) and by 1.0e-4 under std 0.1 (measured on the CPU; 60 frames: 1.6e-3
    and 2.0e-5).  Under std 1 no implementation that differs from the oracle by fp32 rounding meets 1e-3 on the joints (this path:
    2.4e-3 in fp32 mode, 1.4e-2 in f16x3); under std 0.1 the gate holds what the frame gate holds."""
    gen = torch.Generator().manual_seed(97)
    enc_out = torch.randn(6, 1, 768, generator=gen)
    motion = torch.randn(3, 196, 263, generator=gen)
    eps = torch.randn(5, 3, 256, generator=gen)
    strength, seeds = [1.0, 0.5, 0.34], [5, 6, 7]
    model = edit_model(nets, enc_out, "ddpm", precision=precision)
    starts = [model.scheduler.start_step(s, 6) for s in strength]
    assert starts == [0, 3, 4]
    batch = {"text": ["a", "b", "c"], "length": LENS3, "motion": motion.to(DEV)}
    joints = model.edit(batch, strength, seeds=seeds, eps=eps.to(DEV))
    assert model.loop_status() == (0, 0)
    _, _, lat = orc.vae_encode(syn.vae_weights(263), motion, LENS3, eps)
    for i, l in enumerate(LENS3):
        init, steps = edit_ref.generator_noise(seeds[i], 0, POSITIONS["ddpm"], 5)
        _, f_o = oracle(("edit3", i), lambda: edit_ref.edit_prompt(enc_out[[i, 3 + i]], l, lat[:, i], init, starts[i], 6, "ddpm", 7.5, steps))
        j_o = orc.feats2joints(f_o, torch.zeros(263), torch.full((263,), JOINT_STD), 22)[0, :l]
        err, scale = maxdiff(joints[i], j_o), max(1.0, j_o.abs().max().item())
        print(f"{precision} prompt {i} strength {strength[i]} (start {starts[i]}): |joints - oracle| = {err:.2e} (scale {scale:.1f})")
        assert joints[i].shape[0] == l and err < FRAME_TOL


def test_edit_from_latents_of_an_earlier_sample(nets):
    enc_out = torch.randn(6, 1, 768, generator=torch.Generator().manual_seed(97))
    model = edit_model(nets, enc_out, "ddim")
    z, _ = model.sample(enc_out.to(DEV), LENS3, init_noise=syn.init_noise(LENS3, seed=98).to(DEV))
    batch = {"text": ["a", "b", "c"], "length": LENS3}
    joints = model.edit(batch, 0.5, latents=z, seeds=[1, 2, 3])
    again = model.edit(batch, 0.5, latents=z, seeds=[1, 2, 4])
    assert all(torch.isfinite(j).all() and j.shape[0] == l for j, l in zip(joints, LENS3))
    assert torch.equal(again[0], joints[0]) and not torch.equal(again[2], joints[2])       # only the request whose seed changed moves
    zz = model._diffusion_reverse(enc_out.to(DEV), LENS3, seeds=[1, 2, 3], source_latents=z, strength=0.5)
    want = model.feats2joints_device(model.vae.decode(zz, LENS3)).cpu()
    assert all(torch.equal(joints[i], want[i, :l]) for i, l in enumerate(LENS3))


def test_fallback_reruns_an_edit_launch_per_stage(nets):
    text, noise, z0 = case7()
    kw = dict(init_noise=noise, source_latents=z0, start_steps=STARTS7, guidance_scale=SCALES7)
    want = reverse(make_pipe(nets, "launches", "f16x3", "dpm"), "launches", text, LENS7, **kw)
    fb = make_pipe(nets, "pipeline", "f16x3", "dpm", fallback=True)
    try:
        fb.set_pipeline_fault(17, 20)                                  # workgroup 17 leaves at once; waits time out after 20 ms
        with torch.no_grad():
            got = fb._diffusion_reverse(text.to(DEV), LENS7, **{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()})
        torch.cuda.synchronize()
    finally:
        fb.set_pipeline_fault(-1, 0)
    assert fb.fallback_count == 1 and torch.isfinite(got).all()
    err, scale = maxdiff(got, want), max(1.0, want.abs().max().item())
    print(f"fallback re-run against a launch-per-stage call: {err:.2e} (scale {scale:.2f}), bit-equal: {torch.equal(got, want)}")
    assert err < LOOP_TOL["f16x3"] * scale


@pytest.mark.parametrize("precision", MODES)
def test_chunked_batch_slices_sources_and_starts(nets, precision):
    """Two launches of 4 and 3 prompts: each takes its slice of z0 and of the starts, and its own first_step (0 and 2)."""
    text, noise, z0 = case7()
    kw = dict(init_noise=noise, source_latents=z0, start_steps=STARTS7, guidance_scale=SCALES7)
    whole = reverse(make_pipe(nets, "pipeline", precision, "dpm"), "pipeline", text, LENS7, **kw)
    chunked = make_pipe(nets, "pipeline", precision, "dpm", max_prompts_per_launch=4)
    chunks = reverse(chunked, "pipeline", text, LENS7, **kw)
    assert len(chunked._last) == 2
    assert torch.isfinite(chunks).all() and maxdiff(whole, chunks) < LOOP_TOL[precision] * max(1.0, whole.abs().max().item())


# ---------------------------------------------------------------- 10: without a sampler handle
@pytest.mark.parametrize("sched", SCHEDS)
@pytest.mark.parametrize("precision", MODES)
def test_plain_launches_without_a_sampler_take_the_same_arguments(nets, precision, sched):
    text, noise, z0 = case7()
    kw = dict(source_latents=z0, start_steps=STARTS7, guidance_scale=SCALES7, **noise_args(sched, noise))
    with_sampler = reverse(make_pipe(nets, "launches", precision, sched), "launches", text, LENS7, **kw)
    plain_pipe = make_pipe(nets, "launches", precision, sched, use_graph=False)
    with torch.no_grad():
        plain = plain_pipe._diffusion_reverse(text.to(DEV), LENS7, **{k: (v.to(DEV) if torch.is_tensor(v) and v.dim() > 1 else v) for k, v in kw.items()})
    torch.cuda.synchronize()
    assert plain_pipe.loop_status() == (0, 0) and all(p["sampler"] is None for p in plain_pipe._plans.values())
    err, scale = maxdiff(with_sampler, plain), max(1.0, with_sampler.abs().max().item())
    print(f"{sched} {precision}: step graphs against plain launches: {err:.2e} (scale {scale:.2f}), bit-equal: {torch.equal(with_sampler, plain)}")
    assert torch.isfinite(plain).all() and err < LOOP_TOL[precision] * scale
