"""DPMSolverMultistepScheduler on the GPU: the unit entry of the rule against fp64, the three loop forms against the CPU oracle driven by
the fp64 reference of tests/dpm_solver_ref.py, the block geometries of the pipeline kernel, the state buffer across calls, windows,
chunks and per-prompt requests, and the module-level Python loop.  Six steps = one first-order step, four second-order steps, one
first-order step: both branches of every tail run."""
import pytest
import torch

from ladiff_amd import LADIFF, DPMSolverMultistepScheduler, LADiffDenoiser, LADiffVae, _lib, synthetic as syn
from oracle import ladiff_oracle as orc
from dpm_solver_ref import DPMSolverPP2M
from test_abi import ABL, DEN_KW, VAE_KW
from test_gpu_path import FRAME_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DPM_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
LENS7 = [48, 91, 134, 192, 196, 38, 96]                   # latent counts 1 .. 5
LOOP_TOL = {"f16x3": 2e-4, "fp32": 1e-5}                  # launch-per-stage against the pipeline kernel (tests/test_gpu_pipeline.py)
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


def make_pipe(nets, loop, precision, steps=6, T=5, order=2, **kw):
    den, vae = nets
    return LADIFF(denoiser=den, vae=vae, scheduler=DPMSolverMultistepScheduler(solver_order=order, **DPM_KW), guidance_scale=7.5,
                  num_inference_timesteps=steps, eta=0.0, max_it=T, precision=precision, loop=loop, **kw)


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


def oracle_run(tag, text, lens, noise, steps=6, order=2, scale=7.5):
    return oracle((tag, steps, order, float(scale)), lambda: orc.sample_motions(
        syn.denoiser_weights(), syn.vae_weights(263), text, lens, noise, steps, DPMSolverPP2M(solver_order=order), guidance_scale=scale))


def mixed_lengths(B, T):
    return [max(1, min(196, 48 * ((i % T) + 1) - 5 * (i % 3))) for i in range(B)]


# ---------------------------------------------------------------- 1: the unit entry
@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("row", [0, 3, 5])
def test_unit_entry_against_fp64(row, cfg):
    """ladiff_cfg_scheduler_step_multistep on B = 3, T = 5 at rows 0, 3 and the last of the 6-step table.  Row 0 (k_m = 0) finds NaN in
    x0_prev: nothing of it may reach the result.  Inputs: x, eps ~ N(0, 1), guidance 2.0, m1 ~ N(0, 10^2).  The largest intermediate
    is then k_x0 x0 <= ~20 (row 0: x0 <= ~240, k_x0 = 0.07), whose fp32 half-ulps - a few of them along the chain - stay below 5e-6,
    so atol = rtol = 1e-5 also holds where the terms of the sum cancel."""
    B, T, g = 3, 5, 2.0
    sch = DPMSolverMultistepScheduler(**DPM_KW)
    sch.set_timesteps(6)
    tab = sch.coef_table()
    assert (float(tab[row, 6]) != 0.0) == (row == 3)
    gen = torch.Generator().manual_seed(10 * row + cfg)
    x = torch.randn(B, T, 256, generator=gen)
    eps = torch.randn(2 if cfg else 1, B, T, 256, generator=gen)
    m1 = 10.0 * torch.randn(B, T, 256, generator=gen)
    x0p = (torch.full_like(m1, float("nan")) if row == 0 else m1).to(DEV)
    lat, d_step = x.clone().to(DEV), torch.tensor([row], dtype=torch.int32, device=DEV)
    coef, eps_d = tab.to(DEV), eps.to(DEV).contiguous()
    _lib.check(_lib.lib().ladiff_cfg_scheduler_step_multistep(_lib.ptr(eps_d), _lib.ptr(lat), _lib.ptr(x0p), _lib.ptr(coef), d_step.data_ptr(),
                                                              None, g, cfg, B, T, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    sa, sb, kx0, kx, _, _, km = [float(v) for v in tab[row, :7].to(torch.float64)]
    e64 = eps.to(torch.float64)
    e = e64[0] + g * (e64[1] - e64[0]) if cfg else e64[0]
    m0 = (x.to(torch.float64) - sb * e) / sa
    want = kx0 * m0 + kx * x.to(torch.float64) + (km * m1.to(torch.float64) if km != 0.0 else 0.0)
    got, left = lat.cpu().to(torch.float64), x0p.cpu().to(torch.float64)
    print(f"row {row} cfg {cfg}: |latents - fp64| = {(got - want).abs().max().item():.2e} (max {want.abs().max().item():.1f}), "
          f"|x0_prev - fp64| = {(left - m0).abs().max().item():.2e} (max {m0.abs().max().item():.1f})")
    assert torch.isfinite(got).all() and torch.isfinite(left).all()
    assert torch.allclose(got, want, atol=1e-5, rtol=1e-5)
    assert torch.allclose(left, m0, atol=1e-5, rtol=1e-5)


# ---------------------------------------------------------------- 2: the loop against the oracle
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("loop", ["launches", "pipeline16", "pipeline32"])
def test_loop_matches_the_oracle_and_not_its_first_order_run(nets, loop, precision):
    """Seven prompts of latent counts 1 .. 5, 6 steps, guidance 7.5: every prompt's frames are the oracle's under the fp64 reference
    solver - and NOT the oracle's under the same solver at order 1.  The two oracle runs themselves differ by 0.15 .. 0.74 on the frames
    of the seven prompts (frames up to 3.3) at the text seed used (907, the seed of tests/test_gpu_prompt_params.py; measured on the
    CPU) - at least 150 gates - so a tail that dropped or mis-addressed the k_m m1 term cannot pass."""
    text, noise = case7()
    _, feats = sample(make_pipe(nets, loop, precision), text, LENS7, loop, init_noise=noise)
    _, f2 = oracle_run("case7", text, LENS7, noise, order=2)
    _, f1 = oracle_run("case7", text, LENS7, noise, order=1)
    for i, l in enumerate(LENS7):
        sep = maxdiff(f2[i, :l], f1[i, :l])
        own, other = maxdiff(feats[i, :l], f2[i, :l]), maxdiff(feats[i, :l], f1[i, :l])
        print(f"{loop} {precision} prompt {i}: |frames - oracle(2M)| = {own:.2e}, |frames - oracle(order 1)| = {other:.2e}, "
              f"oracle(2M) against oracle(order 1) = {sep:.2e}")
        assert sep >= 10 * FRAME_TOL
        assert own < FRAME_TOL
        assert other >= FRAME_TOL


# ---------------------------------------------------------------- 3: block geometries
_LAUNCHES = {}


@pytest.mark.parametrize("loop", ["pipeline16", "pipeline32", "pipeline"])
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("B,T", [(1, 5), (3, 5), (7, 5), (43, 5), (9, 2), (5, 8)])
def test_every_block_geometry_carries_the_previous_prediction(nets, loop, precision, B, T):
    """(1, 5) is the tail that owns one unit and does not prefetch, (43, 5) gives a tail several units; every (prompt, latent) pair must
    meet its own row of x0_prev, as the launch-per-stage loop's tail launch does row by row."""
    lens = mixed_lengths(B, T)
    text = syn.text_embeddings(B, seed=900 + B)
    noise = torch.randn(B, T, 256, generator=torch.Generator().manual_seed(B * 10 + T))
    if (precision, B, T) not in _LAUNCHES:
        _LAUNCHES[(precision, B, T)] = reverse(make_pipe(nets, "launches", precision, T=T), text, lens, "launches", init_noise=noise)
    za = _LAUNCHES[(precision, B, T)]
    zb = reverse(make_pipe(nets, loop, precision, T=T), text, lens, loop, init_noise=noise)
    scale = max(1.0, za.abs().max().item())
    assert torch.isfinite(zb).all()
    assert maxdiff(za, zb) < LOOP_TOL[precision] * scale
    for i, l in enumerate(lens):                                    # rows past a motion's latent count: exact zeros
        c = -(-l // 48)
        if c < T:
            assert zb[c:, i].abs().max().item() == 0 and za[c:, i].abs().max().item() == 0


# ---------------------------------------------------------------- 4: the state buffer between calls
@pytest.mark.parametrize("loop", ["launches", "pipeline16", "pipeline32"])
def test_state_does_not_leak_between_calls(nets, loop):
    text, noise = case7()
    other = syn.text_embeddings(7, seed=31)
    pipe = make_pipe(nets, loop, "f16x3")
    z0 = reverse(pipe, text, LENS7, loop, init_noise=noise)
    assert torch.isfinite(z0).all()
    assert torch.equal(reverse(pipe, text, LENS7, loop, init_noise=noise), z0)
    assert not torch.equal(reverse(pipe, other, LENS7, loop, init_noise=noise), z0)     # leaves other rows in x0_prev
    assert torch.equal(reverse(pipe, text, LENS7, loop, init_noise=noise), z0)
    assert len(pipe._plans) == 1
    next(iter(pipe._plans.values()))["x0_prev"].fill_(float("nan"))                     # whatever the buffer holds on entry
    assert torch.equal(reverse(pipe, text, LENS7, loop, init_noise=noise), z0)


# ---------------------------------------------------------------- 5: two windows
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_previous_prediction_survives_the_window_boundary(nets, precision):
    """66 steps run as two pipeline launches of 33: step 33 is a second-order step whose m1 was written by the launch before."""
    B, T, n = 3, 5, 66
    lens, text = [196, 60, 130], syn.text_embeddings(3, seed=43)
    noise = syn.init_noise(lens, seed=44)
    pipe = make_pipe(nets, "pipeline", precision, steps=n)
    pipe.window_ms(enable=True)
    zp = reverse(pipe, text, lens, "pipeline", init_noise=noise)
    assert pipe.window_ms()[1] == 2
    plain = make_pipe(nets, "launches", precision, steps=n, use_graph=False)
    zl = plain._diffusion_reverse(text.to(DEV), lens, init_noise=noise.to(DEV))
    assert plain.loop_status() == (0, 0)
    err, scale = maxdiff(zp, zl), max(1.0, zl.abs().max().item())
    print(f"{precision}: 66 steps, pipeline against plain launches: {err:.2e} (scale {scale:.2f})")
    assert torch.isfinite(zp).all() and err < LOOP_TOL[precision] * scale


# ---------------------------------------------------------------- 6: with per-prompt requests
@pytest.mark.parametrize("loop", ["launches", "pipeline16", "pipeline32"])
def test_per_prompt_guidance_with_the_multistep_rule(nets, loop):
    lens, scales = [196, 60, 130], [2.0, 7.5, 4.5]
    text, noise = syn.text_embeddings(3, seed=43), syn.init_noise([196, 60, 130], seed=44)
    _, feats = sample(make_pipe(nets, loop, "f16x3"), text, lens, loop, init_noise=noise, guidance_scale=scales)
    for i, (l, g) in enumerate(zip(lens, scales)):
        _, f_o = oracle_run(("three", i), text[[i, 3 + i]], [l], noise[i:i + 1], scale=g)
        err = maxdiff(feats[i, :l], f_o[0, :l])
        print(f"{loop} prompt {i} scale {g}: |frames - oracle| = {err:.2e}")
        assert err < FRAME_TOL


# ---------------------------------------------------------------- 7: chunks
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_chunked_batch_equals_the_whole_batch(nets, precision):
    text, noise = case7()
    whole = reverse(make_pipe(nets, "pipeline", precision), text, LENS7, "pipeline", init_noise=noise)
    chunked = make_pipe(nets, "pipeline", precision, max_prompts_per_launch=4)
    chunks = reverse(chunked, text, LENS7, "pipeline", init_noise=noise)
    assert len(chunked._last) == 2 and all("x0_prev" in p for p in chunked._last)
    assert maxdiff(whole, chunks) < LOOP_TOL[precision] * max(1.0, whole.abs().max().item())


# ---------------------------------------------------------------- 8: the module-level Python loop
def test_module_level_loop_matches_fused_loop(nets):
    """The reference's loop over the drop-in modules - denoiser(...), scheduler.step(...).prev_sample - with the stateful scheduler."""
    den, _ = nets
    text, noise = case7()
    z = reverse(make_pipe(nets, "pipeline", "fp32"), text, LENS7, "pipeline", init_noise=noise)
    sch = DPMSolverMultistepScheduler(**DPM_KW)
    sch.set_timesteps(6)
    counts = torch.tensor(syn.max_iter_elements(LENS7))
    lat, txt = noise.to(DEV), text.to(DEV)
    for t in sch.timesteps:
        eps = den(torch.cat([lat] * 2), t, txt, lengths=LENS7 * 2, max_iter_elements=torch.cat([counts] * 2))[0]
        eu, ec = eps.chunk(2)
        lat = sch.step(eu + 7.5 * (ec - eu), t, lat).prev_sample
    lat = lat.permute(1, 0, 2).clone()
    for i, m in enumerate(counts.tolist()):
        lat[m:, i] = 0
    err, scale = maxdiff(z, lat), max(1.0, lat.abs().max().item())
    print(f"module-level loop against the fused loop: {err:.2e} (scale {scale:.2f})")
    assert err < LOOP_TOL["fp32"] * scale
    sch.set_timesteps(6)                                            # the state is gone: the schedule starts again at step 0
    assert sch._x0_prev is None and sch._step_index is None


# ---------------------------------------------------------------- 9: more than one text token
def test_two_text_tokens_take_the_buffer_through_the_tail_launch(nets):
    B, lens = 3, [196, 60, 130]
    gen = torch.Generator().manual_seed(404)
    text, noise = torch.randn(2 * B, 2, 768, generator=gen), syn.init_noise(lens, seed=405)
    pipe = make_pipe(nets, "pipeline", "fp32")
    _, feats = sample(pipe, text, lens, "launches", init_noise=noise)       # n_text > 1 runs launch per stage whatever was asked for
    _, f_o = oracle_run("n_text2", text, lens, noise)
    for i, l in enumerate(lens):
        err = maxdiff(feats[i, :l], f_o[i, :l])
        print(f"n_text 2 prompt {i}: |frames - oracle| = {err:.2e}")
        assert err < FRAME_TOL
