"""The denoising trajectory on the GPU: the unit entry of the rule with its record against fp64; every loop form, mode
and scheduler against the CPU oracle's recording (tests/trajectory_ref.py), row by row, with the off-by-one and swap checks the oracle's
own separation allows; the bits a recording must not change; the block geometries of the pipeline kernel; windows; an edit's frozen and
live rows; plans and chunks; `decode_trajectory`, `preview` and the reference's `_diffusion_reverse_tsne`.  Synthetic weights, T = 5,
6 steps = one first-order step, four second-order steps and one first-order step under the 2M rule (tests/test_gpu_dpm_solver.py)."""
from types import SimpleNamespace

import pytest
import torch

from ladiff_amd import LADIFF, DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, LADiffDenoiser, LADiffVae, _lib, synthetic as syn
from oracle import ladiff_oracle as orc
import edit_ref
import trained_like
import trajectory_ref as ref
from test_abi import ABL, DEN_KW, VAE_KW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
LENS7 = ref.LENS7
LOOP_TOL = {"f16x3": 2e-4, "fp32": 1e-5}                  # launch-per-stage against the pipeline kernel (tests/test_gpu_pipeline.py)
MODES = ["fp32", "f16x3"]
STARTS3 = [0, 4, 2]
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


def make_pipe(nets, loop, precision, sched="ddim", steps=6, T=5, **kw):
    den, vae = nets
    return LADIFF(denoiser=den, vae=vae, scheduler=scheduler(sched), guidance_scale=7.5, num_inference_timesteps=steps, eta=0.0, max_it=T,
                  precision=precision, loop=loop, **kw)


def to_dev(kw):
    return {k: (v.to(DEV) if torch.is_tensor(v) and v.dim() > 1 else v) for k, v in kw.items()}


def reverse(pipe, text, lens, loop=None, **kw):
    with torch.no_grad():
        out = pipe._diffusion_reverse(text.to(DEV), lens, **to_dev(kw))
        torch.cuda.synchronize()
    assert pipe.loop_status() == (0, 0)
    if loop is not None:
        assert pipe.last_loop()[0] == (loop != "launches")
    return out


def maxdiff(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def mixed_lengths(B, T):
    return [max(1, min(196, 48 * ((i % T) + 1) - 5 * (i % 3))) for i in range(B)]


def padded_rows_are_zero(rows, lens, T=5):
    """rows [S,T,B,256]: the rows past each prompt's latent count are exact zeros at every position."""
    for i, l in enumerate(lens):
        c = -(-l // 48)
        if c < T and rows[:, c:, i].abs().max().item() != 0:
            return False
    return True


# ---------------------------------------------------------------- 1: the unit entry against fp64
@pytest.mark.parametrize("row", [0, 3, 5])
@pytest.mark.parametrize("table", ["ddim", "ddim_eta1", "dpm"])
def test_unit_entry_records_its_row_against_fp64(table, row):
    """ladiff_cfg_scheduler_step_record on B = 3, T = 5 with starts 0 4 2 at rows 0, 3 and 5 of the 6-step table: prompt 1 is frozen at
    rows 0 and 3, prompt 2 at row 0.  Inputs and bound as tests/test_gpu_dpm_solver.py::test_unit_entry_against_fp64 (x, eps, noise ~
    N(0, 1), guidance 2.0, m1 ~ N(0, 10^2): atol = rtol = 1e-5).  Both trajectory buffers hold NaN on entry: only row `row` may change."""
    B, T, g, n = 3, 5, 2.0, 6
    sch = scheduler("dpm" if table == "dpm" else "ddim")
    sch.set_timesteps(n)
    tab = sch.coef_table(1.0) if table == "ddim_eta1" else sch.coef_table()
    multistep = table == "dpm"
    gen = torch.Generator().manual_seed(100 + row)
    x = torch.randn(B, T, 256, generator=gen)
    eps = torch.randn(2, B, T, 256, generator=gen)
    m1 = 10.0 * torch.randn(B, T, 256, generator=gen)
    noise = torch.randn(n, B, T, 256, generator=gen) if table == "ddim_eta1" else None
    x0p = (torch.full_like(m1, float("nan")) if row == 0 else m1).to(DEV) if multistep else None
    x0p_before = None if x0p is None else x0p.cpu().view(torch.int32).clone()           # by bits: row 0 finds NaN there
    lat, d_step = x.clone().to(DEV), torch.tensor([row], dtype=torch.int32, device=DEV)
    starts = torch.tensor(STARTS3, dtype=torch.int32, device=DEV)
    coef, eps_d = tab.to(DEV), eps.to(DEV).contiguous()
    noise_d = None if noise is None else noise.to(DEV)
    tx = torch.full((n, B, T, 256), float("nan"), device=DEV)
    tx0 = torch.full((n, B, T, 256), float("nan"), device=DEV)
    _lib.check(_lib.lib().ladiff_cfg_scheduler_step_record(
        _lib.ptr(eps_d), _lib.ptr(lat), None if x0p is None else _lib.ptr(x0p), _lib.ptr(coef), d_step.data_ptr(),
        None if noise_d is None else _lib.ptr(noise_d), g, 1, B, T, starts.data_ptr(), 0, _lib.ptr(tx), _lib.ptr(tx0),
        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    tx, tx0, lat = tx.cpu(), tx0.cpu(), lat.cpu()
    for s in range(n):                                             # rows of other positions still hold NaN
        if s != row:
            assert torch.isnan(tx[s]).all() and torch.isnan(tx0[s]).all()
    assert torch.equal(tx[row], lat)                               # the bits stored to the latents
    sa, sb, kx0, kx, ke, kn, km = [float(v) for v in tab[row, :7].to(torch.float64)]
    e64 = eps.to(torch.float64)
    e = e64[0] + g * (e64[1] - e64[0])
    for b, start in enumerate(STARTS3):
        if row < start:                                            # frozen: the latents as they stand, a zero prediction, m1 untouched
            assert torch.equal(lat[b], x[b]) and tx0[row, b].abs().max().item() == 0
            if multistep:
                assert torch.equal(x0p.cpu().view(torch.int32)[b], x0p_before[b])
            continue
        k0, k_m = (kx0 + km, 0.0) if (multistep and row == start) else (kx0, km if multistep else 0.0)
        m0 = (x[b].to(torch.float64) - sb * e[b]) / sa
        want = k0 * m0 + kx * x[b].to(torch.float64) + ke * e[b]
        if kn != 0.0 and noise is not None:
            want = want + kn * noise[row, b].to(torch.float64)
        if k_m != 0.0:
            want = want + k_m * m1[b].to(torch.float64)
        ex, ex0 = (tx[row, b].double() - want).abs().max().item(), (tx0[row, b].double() - m0).abs().max().item()
        print(f"{table} row {row} prompt {b}: |traj_x - fp64| = {ex:.2e} (max {want.abs().max().item():.1f}), |traj_x0 - fp64| = {ex0:.2e} "
              f"(max {m0.abs().max().item():.1f})")
        assert torch.allclose(tx[row, b].double(), want, atol=1e-5, rtol=1e-5)
        assert torch.allclose(tx0[row, b].double(), m0, atol=1e-5, rtol=1e-5)
        if multistep:
            assert torch.equal(x0p.cpu()[b], tx0[row, b])
    if table == "ddim_eta1":
        assert kn != 0.0
    # either pointer may be null: the other kind alone, same bits
    lat2, only = x.clone().to(DEV), torch.full((n, B, T, 256), float("nan"), device=DEV)
    x0p2 = (torch.full_like(m1, float("nan")) if row == 0 else m1).to(DEV) if multistep else None
    _lib.check(_lib.lib().ladiff_cfg_scheduler_step_record(
        _lib.ptr(eps_d), _lib.ptr(lat2), None if x0p2 is None else _lib.ptr(x0p2), _lib.ptr(coef), d_step.data_ptr(),
        None if noise_d is None else _lib.ptr(noise_d), g, 1, B, T, starts.data_ptr(), 0, None, _lib.ptr(only),
        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(lat2.cpu(), lat) and torch.equal(only.cpu()[row], tx0[row])


# ---------------------------------------------------------------- 2: every row against the oracle
@pytest.mark.parametrize("sched", ["ddim", "dpm"])
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("loop", ["launches", "pipeline16", "pipeline32"])
def test_every_row_matches_the_oracle_and_not_its_neighbours(nets, loop, precision, sched):
    """Seven prompts of latent counts 1 .. 5, 6 steps, guidance 7.5.  Row s of either kind is within trained_like.bound(e32[s], want[s])
    of the fp64 recording (e32: the oracle's own fp32 error of that row), and - prompt by prompt, on its valid rows - NOT within it of
    the oracle's rows s - 1 and s + 1 nor of the other kind's row s: an off-by-one position or swapped buffers cannot pass.  The oracle's
    own separation is asserted first (>= 10 bounds; measured on the CPU: DDIM consecutive rows >= 0.31 (latents) and 0.38 (x0), |x - x0|
    >= 0.69 against an f16x3 bound <= 0.018; DPM >= 34 and 5.0 against <= 0.051).  The last DPM row's latents ARE its data prediction
    (sigma = 0): no swap check there."""
    text, noise = ref.case7()
    xs, x0s, ex, ex0 = ref.oracle_case7(sched)
    sep = ref.separation(sched, precision)
    z, traj = reverse(make_pipe(nets, loop, precision, sched), text, LENS7, loop, init_noise=noise, trajectory="both")
    assert traj["first_step"] == 0 and traj["latents"].shape == traj["x0"].shape == (6, 5, 7, 256)
    got_x, got_x0 = traj["latents"].cpu().double(), traj["x0"].cpu().double()
    assert torch.isfinite(got_x).all() and torch.isfinite(got_x0).all()
    far = lambda a, b, i: (ref.prompt_rows(a, i) - ref.prompt_rows(b, i)).abs().max().item()
    for s in range(6):
        d = sep[s]
        last_dpm = sched == "dpm" and s == 5
        assert d["near_x"] >= 10 * d["bx"] and d["near_x0"] >= 10 * d["bx0"] and (last_dpm or d["swap"] >= 10 * max(d["bx"], d["bx0"]))
        err_x, err_x0 = maxdiff(got_x[s], xs[s]), maxdiff(got_x0[s], x0s[s])
        print(f"{loop} {precision} {sched} position {s}: |latents - oracle| = {err_x:.2e} (bound {d['bx']:.2e}, e32 {ex[s]:.1e}, max "
              f"{xs[s].abs().max().item():.1f}), |x0 - oracle| = {err_x0:.2e} (bound {d['bx0']:.2e}, e32 {ex0[s]:.1e}, max {x0s[s].abs().max().item():.1f})")
        assert err_x < d["bx"] and err_x0 < d["bx0"]
        for i in range(7):
            for t in (s - 1, s + 1):
                if 0 <= t < 6:
                    assert far(got_x[s], xs[t], i) >= d["bx"] and far(got_x0[s], x0s[t], i) >= d["bx0"]
            if not last_dpm:
                assert far(got_x[s], x0s[s], i) >= d["bx"] and far(got_x0[s], xs[s], i) >= d["bx0"]
    assert padded_rows_are_zero(traj["latents"], LENS7) and padded_rows_are_zero(traj["x0"], LENS7)


# ---------------------------------------------------------------- 3: the bits a recording must not change
@pytest.mark.parametrize("sched", ["ddim", "ddpm", "dpm"])
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("loop", ["launches", "pipeline16", "pipeline32", "pipeline"])
def test_recording_changes_no_bit(nets, loop, precision, sched):
    """z and the frames of a recording call are those of the same call without; the last latents row is z; padded rows are exact zeros.
    DDPM draws its step noise on the device from `noise_seed`."""
    text, noise = ref.case7()
    pipe = make_pipe(nets, loop, precision, sched)
    kw = dict(init_noise=noise.to(DEV), noise_seed=4242)
    with torch.no_grad():
        z_r, f_r, traj = pipe.sample(text.to(DEV), LENS7, trajectory="both", **kw)
        assert pipe.loop_status() == (0, 0) and pipe.last_loop()[0] == (loop != "launches")
        z_p, f_p = pipe.sample(text.to(DEV), LENS7, **kw)
        assert pipe.loop_status() == (0, 0) and pipe.last_loop()[0] == (loop != "launches")
        z_x, traj_x = reverse(pipe, text, LENS7, loop, trajectory="latents", **kw)
    n = 7 if sched == "ddpm" else 6                                 # DDPMScheduler.set_timesteps(6): seven positions
    assert traj["latents"].shape == traj["x0"].shape == (n, 5, 7, 256) and set(traj_x) == {"latents", "first_step"}
    assert torch.isfinite(z_r).all() and torch.equal(z_r, z_p) and torch.equal(f_r, f_p) and torch.equal(z_x, z_p)
    assert torch.equal(traj["latents"][-1], z_r) and torch.equal(traj_x["latents"], traj["latents"])
    assert torch.isfinite(traj["latents"]).all() and torch.isfinite(traj["x0"]).all()
    assert padded_rows_are_zero(traj["latents"], LENS7) and padded_rows_are_zero(traj["x0"], LENS7)
    assert not torch.equal(traj["latents"][0], traj["latents"][1]) and not torch.equal(traj["x0"][0], traj["latents"][0])


# ---------------------------------------------------------------- 4: block geometries
_LAUNCHES = {}


@pytest.mark.parametrize("loop", ["pipeline16", "pipeline32"])
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("B,T", [(1, 5), (3, 5), (7, 5), (43, 5), (9, 2), (5, 8)])
def test_every_block_geometry_records_every_pair(nets, loop, precision, B, T):
    """(1, 5) is the tail that owns one unit, (43, 5) gives a tail several: every (prompt, latent) pair must store its own rows, as the
    launch-per-stage tail does row by row (the 2M rule: the record and x0_prev travel together).  The plan's buffers hold NaN on entry:
    afterwards every element is finite, and an exact zero in a padded row."""
    lens = mixed_lengths(B, T)
    text = syn.text_embeddings(B, seed=900 + B)
    noise = torch.randn(B, T, 256, generator=torch.Generator().manual_seed(B * 10 + T))

    def run(form):
        pipe = make_pipe(nets, form, precision, "dpm", T=T)
        plan = pipe._get_plan(B, T, 6, 0.0, torch.device(DEV), 1, "both")
        plan["traj_x"].fill_(float("nan")); plan["traj_x0"].fill_(float("nan"))
        out = reverse(pipe, text, lens, form, init_noise=noise, trajectory="both")
        assert len(pipe._plans) == 1
        return out
    if (precision, B, T) not in _LAUNCHES:
        _LAUNCHES[(precision, B, T)] = run("launches")
    (za, ta), (zb, tb) = _LAUNCHES[(precision, B, T)], run(loop)
    assert torch.equal(tb["latents"][-1], zb) and torch.equal(ta["latents"][-1], za)
    for kind in ("latents", "x0"):
        for t in (ta, tb):
            assert t[kind].shape == (6, T, B, 256) and torch.isfinite(t[kind]).all() and padded_rows_are_zero(t[kind], lens, T)
        for s in range(6):
            scale = max(1.0, ta[kind][s].abs().max().item())
            assert maxdiff(ta[kind][s], tb[kind][s]) < LOOP_TOL[precision] * scale, (kind, s)


# ---------------------------------------------------------------- 5: two windows
@pytest.mark.parametrize("precision", MODES)
def test_rows_keep_their_global_position_across_windows(nets, precision):
    """66 steps run as two pipeline launches of 33: row 33 is written by the second launch, at its global index."""
    n, lens, text = 66, [196, 60, 130], syn.text_embeddings(3, seed=43)
    noise = syn.init_noise(lens, seed=44)
    pipe = make_pipe(nets, "pipeline", precision, "dpm", steps=n)
    pipe.window_ms(enable=True)
    zp, tp = reverse(pipe, text, lens, "pipeline", init_noise=noise, trajectory="both")
    assert pipe.window_ms()[1] == 2
    plain = make_pipe(nets, "launches", precision, "dpm", steps=n, use_graph=False)
    zl, tl = reverse(plain, text, lens, None, init_noise=noise, trajectory="both")
    assert torch.equal(tp["latents"][-1], zp) and torch.equal(tl["latents"][-1], zl)
    for kind in ("latents", "x0"):
        assert tp[kind].shape == (n, 5, 3, 256) and torch.isfinite(tp[kind]).all() and padded_rows_are_zero(tp[kind], lens)
        worst = 0.0
        for s in range(n):
            err, scale = maxdiff(tp[kind][s], tl[kind][s]), max(1.0, tl[kind][s].abs().max().item())
            worst = max(worst, err / scale)
            assert err < LOOP_TOL[precision] * scale, (kind, s)
        print(f"{precision} {kind}: 66 rows, pipeline against plain launches: worst {worst:.2e} of the row's scale")
    assert not torch.equal(tp["latents"][32], tp["latents"][33])


# ---------------------------------------------------------------- 6: an edit
@pytest.mark.parametrize("sched", ["ddim", "dpm"])
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("loop", ["launches", "pipeline"])
def test_edit_records_frozen_and_live_rows(nets, loop, precision, sched):
    """Three prompts starting at 0, 4 and 2.  While frozen a prompt's latents rows are edit_ref.noised(...) (test 1's tolerance) and its
    x0 rows zero; from its start on both kinds follow the oracle restarted there under the recording scheduler.  A recording edit runs as
    step graphs whatever loop was asked for: last_loop() says so."""
    lens = [196, 60, 130]
    text, noise = syn.text_embeddings(3, seed=43), syn.init_noise(lens, seed=44)
    z0 = torch.randn(5, 3, 256, generator=torch.Generator().manual_seed(2024))
    for i, l in enumerate(lens):
        z0[-(-l // 48):, i] = 0
    pipe = make_pipe(nets, loop, precision, sched)
    z, traj = reverse(pipe, text, lens, "launches", init_noise=noise, source_latents=z0, start_steps=STARTS3, trajectory="both")
    assert pipe.last_loop()[0] is False
    assert traj["first_step"] == 0 and traj["latents"].shape == (6, 5, 3, 256) and torch.equal(traj["latents"][-1], z)
    z_plain = reverse(pipe, text, lens, loop, init_noise=noise, source_latents=z0, start_steps=STARTS3)
    assert maxdiff(z, z_plain) < LOOP_TOL[precision] * max(1.0, z_plain.abs().max().item())     # the pipeline's own edit, another loop form
    if loop == "launches":
        assert torch.equal(z, z_plain)
    for i, (l, start) in enumerate(zip(lens, STARTS3)):
        c = -(-l // 48)
        frozen = edit_ref.noised(sched, 6, start, z0[:, i], noise[i])
        for s in range(start):
            assert torch.allclose(traj["latents"][s, :c, i].cpu(), frozen[:c], atol=1e-5, rtol=1e-5)
            assert traj["x0"][s, :, i].abs().max().item() == 0
        (wx, wx0), e32 = oracle((sched, i), lambda: edit_oracle(sched, text[[i, 3 + i]], l, z0[:, i], noise[i], start))
        for k, s in enumerate(range(start, 6)):
            bx = trained_like.bound(e32[k], wx[k], precision)
            bx0 = trained_like.bound(e32[6 - start + k], wx0[k], precision)
            ex, ex0 = maxdiff(traj["latents"][s, :, i], wx[k, :, 0]), maxdiff(traj["x0"][s, :, i], wx0[k, :, 0])
            print(f"{loop} {precision} {sched} prompt {i} start {start} position {s}: |latents - oracle| = {ex:.2e} (bound {bx:.2e}), "
                  f"|x0 - oracle| = {ex0:.2e} (bound {bx0:.2e})")
            assert ex < bx and ex0 < bx0
    assert padded_rows_are_zero(traj["latents"], lens) and padded_rows_are_zero(traj["x0"], lens)


def edit_oracle(sched, text_rows, length, z0, noise, start):
    """One prompt's live rows under the recording scheduler in fp64, and the fp32 error of every row (latents rows, then x0 rows)."""
    def fn(dtype, sd):
        init = edit_ref.noised(sched, 6, start, z0, noise)[None]
        f = lambda x, t, txt, counts: orc.denoiser_forward(sd, x, t, txt, counts)
        sch = ref.scheduler_from(sched, start)
        orc.diffusion_reverse(f, sch, text_rows.to(dtype), [length], init.to(dtype), 6, guidance_scale=7.5)
        xs, x0s = ref._rows(sch.rec_x, [length], 5), ref._rows(sch.rec_x0, [length], 5)
        return tuple(xs) + tuple(x0s)
    want, e32 = trained_like.oracle_pair(fn, syn.denoiser_weights())
    m = len(want) // 2
    return (torch.stack(want[:m]), torch.stack(want[m:])), e32


# ---------------------------------------------------------------- 7: plans, replays, chunks
@pytest.mark.parametrize("loop", ["launches", "pipeline16", "pipeline32"])
def test_plans_do_not_leak_between_recording_and_plain_calls(nets, loop):
    text, noise = ref.case7()
    other = syn.text_embeddings(7, seed=31)
    pipe = make_pipe(nets, loop, "f16x3", "dpm")
    z1, t1 = reverse(pipe, text, LENS7, loop, init_noise=noise, trajectory="both")
    z2 = reverse(pipe, text, LENS7, loop, init_noise=noise)
    z3, t3 = reverse(pipe, other, LENS7, loop, init_noise=noise, trajectory="both")
    z4, t4 = reverse(pipe, text, LENS7, loop, init_noise=noise, trajectory="both")
    assert torch.equal(z2, z1) and torch.equal(z4, z1) and not torch.equal(z3, z1)
    assert torch.equal(t4["latents"], t1["latents"]) and torch.equal(t4["x0"], t1["x0"]) and not torch.equal(t3["x0"], t1["x0"])
    assert len(pipe._plans) == 2                                   # one plan per kind asked for: None and "both"
    for plan in pipe._plans.values():                              # whatever the buffers hold on entry
        for name in ("traj_x", "traj_x0", "x0_prev"):
            if name in plan:
                plan[name].fill_(float("nan"))
    z5, t5 = reverse(pipe, text, LENS7, loop, init_noise=noise, trajectory="both")
    assert torch.equal(z5, z1) and torch.equal(t5["latents"], t1["latents"]) and torch.equal(t5["x0"], t1["x0"])
    assert len(pipe._plans) == 2


@pytest.mark.parametrize("precision", MODES)
def test_chunked_batch_is_the_concatenation_of_its_chunks(nets, precision):
    """Five prompts in chunks of two (2 + 2 + 1): the record is the chunks' own records side by side."""
    lens = LENS7[:5]
    text, noise = syn.text_embeddings(5, seed=907), syn.init_noise(lens, seed=77)
    chunked = make_pipe(nets, "pipeline", precision, "dpm", max_prompts_per_launch=2)
    z, traj = reverse(chunked, text, lens, "pipeline", init_noise=noise, trajectory="both")
    assert len(chunked._last) == 3 and traj["latents"].shape == (6, 5, 5, 256)
    single = make_pipe(nets, "pipeline", precision, "dpm")
    for lo, hi in ((0, 2), (2, 4), (4, 5)):
        rows = list(range(lo, hi)) + list(range(5 + lo, 5 + hi))
        zc, tc = reverse(single, text[rows], lens[lo:hi], "pipeline", init_noise=noise[lo:hi], trajectory="both")
        assert torch.equal(z[:, lo:hi], zc)
        assert torch.equal(traj["latents"][:, :, lo:hi], tc["latents"]) and torch.equal(traj["x0"][:, :, lo:hi], tc["x0"])


# ---------------------------------------------------------------- 8: decode_trajectory and preview
@pytest.mark.parametrize("precision", MODES)
def test_decode_trajectory_against_the_oracle_decoder(nets, precision):
    """Frames of position s against the fp64 oracle decoder of the product's own row s (x0 rows; a subset of the positions too)."""
    lens = [196, 60, 130]
    text, noise = syn.text_embeddings(3, seed=43), syn.init_noise(lens, seed=44)
    pipe = make_pipe(nets, "pipeline", precision)
    _, traj = reverse(pipe, text, lens, "pipeline", init_noise=noise, trajectory="x0")
    with torch.no_grad():
        frames = pipe.decode_trajectory(traj["x0"], lens)
        some = pipe.decode_trajectory(traj["x0"], lens, steps=[5, 0])
        pipe.trajectory_decode_samples = 6                         # two positions per decode: the same frames
        cut = pipe.decode_trajectory(traj["x0"], lens)
    assert frames.shape == (6, 3, 196, 263) and some.shape == (2, 3, 196, 263) and cut.shape == frames.shape
    rows = traj["x0"].cpu()
    for s in range(6):
        want, e32 = trained_like.oracle_pair(lambda dt, sd: orc.vae_decode(sd, rows[s].to(dt), lens), syn.vae_weights(263))
        b = trained_like.bound(e32[0], want[0], precision)
        takes = [frames[s], cut[s]] + [some[k] for k, t in enumerate((5, 0)) if t == s]
        worst = 0.0
        for got in takes:
            for i, l in enumerate(lens):
                err = maxdiff(got[i, :l], want[0][i, :l])
                worst = max(worst, err)
                assert err < b, (s, i, err, b)
                assert l == 196 or got[i, l:].abs().max().item() == 0
        print(f"{precision} position {s}: |frames - oracle decode| = {worst:.2e} (bound {b:.2e}, e32 {e32[0]:.1e})")


def test_preview_ends_at_forwards_joints(nets):
    """previews[-1] of kind "latents" decodes the row that IS z: forward's joints within the feats2joints golden tolerance (2e-5 x scale)."""
    den, vae = nets
    mean, std = torch.zeros(263), torch.ones(263)
    dm = SimpleNamespace(feats2joints=None, hparams=SimpleNamespace(mean=mean.numpy(), std=std.numpy()), njoints=22)
    enc = lambda texts: torch.randn(len(texts), 1, 768, generator=torch.Generator().manual_seed(3)).to(DEV)
    model = LADIFF(None, dm, denoiser=den, vae=vae, text_encoder=enc, guidance_scale=7.5, num_inference_timesteps=5, precision="fp32",
                   scheduler=scheduler("ddim"))
    batch = {"text": ["walk", "run"], "length": [50, 196], "seed": [11, 12]}
    joints = model(batch)
    again, previews = model.preview(batch, kind="latents")
    assert len(previews) == 5 and [tuple(j.shape) for j in previews[0]] == [(50, 22, 3), (196, 22, 3)]
    for b in range(2):
        scale = max(1.0, joints[b].abs().max().item())
        assert torch.equal(again[b], joints[b])
        assert maxdiff(previews[-1][b], joints[b]) < 2e-5 * scale
        assert maxdiff(previews[0][b], joints[b]) > 2e-5 * scale
    _, film = model.preview(batch, steps=[0, 4])                   # the default kind: each step's data prediction
    assert len(film) == 2 and all(torch.isfinite(j).all() for k in film for j in k)


# ---------------------------------------------------------------- 9: the reference's name
def test_tsne_entry_is_the_reshaped_latents(nets):
    text, noise = ref.case7()
    pipe = make_pipe(nets, "pipeline", "f16x3")
    torch.manual_seed(5)
    with torch.no_grad():
        rows = pipe._diffusion_reverse_tsne(text.to(DEV), LENS7)
        torch.manual_seed(5)
        z, traj = pipe._diffusion_reverse(text.to(DEV), LENS7, trajectory="latents")
    assert rows.shape == (6 * 5, 7, 256) and torch.equal(rows, traj["latents"].reshape(30, 7, 256)) and torch.equal(rows[-5:], z)
