"""The denoiser with a text SEQUENCE per prompt (N > 1 tokens: `clip_hidden` / `bert` conditioning, mld_clip.py:80-86) against the fp64
oracle over the token counts, latent counts, row counts, masks and loop forms that decide which code runs.

N > 1 takes the denoiser onto code no other route runs: csrc/linear_ca.hip (lca_kv_kernel: softmax over the N tokens per feature;
lca_apply_kernel: softmax over the 64 features per head, padded rows' query zeroed; den_self_attn_general_kernel: T + N + 1 keys),
denoiser_text_cache_general, the `ntxt > 1` branches of denoiser_forward (split mode: the launch_split_rows twins and a Ys twin written by
a plain GEMM) and, in the loop, launch per stage whatever loop was asked for, with open_window a no-op.

Cases: tests/ntext_cases.py.  Every case runs on both weight sets (plain: indexing and masks show at full size; trained-like: peaked
softmaxes, spread LayerNorms) and in both precisions against the oracle (oracle/ladiff_oracle.py) evaluated at test time in fp64 and
fp32, within trained_like.bound (fp32: 8 e32 + 1e-6 scale; split mode 8 x (fp16 pairs) / 256 x (bf16 pairs) the e32 term; e32 = the
oracle's own fp32-vs-fp64 difference of the case); decoded frames also within the 1e-3 gate, under the condition
test_gpu_trained_like.check applies it.  On these cases a dropped last token, a token taken from the neighbouring prompt, a count read
from the neighbouring sample, a padded query left in place and the tables of a neighbouring step each move a sample by > 10 x the f16x3
bound (tests/test_ntext_cases.py).  `pytest -s` prints err, e32, err / e32 and the bound of every result.

  forward     every case through LADiffDenoiser.forward; the garbage case: 1e30 in the padded latent rows leaves the valid rows' bits
  unit entry  ladiff_linear_cross_attention (fp32), layers 0 / 4 / 8, N = 1 / 2 / 77, T = 1 / 8, B = 3, masked
  loop        LADIFF.sample, latents and frames: guided 5-step DDIM at N = 2 / 77, no guidance at N = 3 (the counts index the undoubled
              batch), use_graph=False, five prompts in chunks of two (also against the unchunked call), DDPM over more than one window of
              steps with the noise drawn on the device.  The trained-like weights run the DDIM cases of one launch only: the long DDPM
              chain on peaked weights amplifies the oracle's own fp32 error past any useful gate, and the chunked case repeats the plain
              one's sequencing.
  refusals    N = 78 through the forward and the loop, an edit with N = 2, per-sample timesteps with N = 2: raised before any launch
              changes a result (the C entries' own codes: tests/test_edit.py::test_argument_errors_return_before_any_gpu_call and
              tests/test_diffusion_stage.py::test_argument_errors_need_no_gpu assert LADIFF_ERR_UNSUPPORTED for n_text = 2; here: the
              callers' surface)

Measured on an MI355X with the fp16-pair library (the bound is 8 in fp32 mode and 64 in f16x3, plus 1e-6 scale): the worst err / e32 is
3.52 in fp32 mode (N = 63, trained-like) and 7.26 in f16x3 (N = 3, trained-like); per group and weight set in DESIGN.md §6.  Against the
library of the commit before this file every case passed: no defect found.  A trial library with two deliberate faults in
csrc/linear_ca.hip (padded query kept; last text key dropped above 64 tokens) failed 122 of the 182 tests, exactly those the faults reach.
The whole file takes 13 s, 7 s of it the CPU oracle.
"""
import zlib

import pytest
import torch

from ladiff_amd import LADIFF, DDIMScheduler, DDPMScheduler, LADiffDenoiser, LADiffVae, _lib, synthetic as syn
from oracle import ladiff_oracle as orc
from test_abi import ABL, DEN_KW, VAE_KW
import test_gpu_trained_like as tl
from test_gpu_trained_like import FRAME_TOL, SCHED_KW, check, oracle

import ntext_cases as nc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = ["fp32", "f16x3"]
KINDS = list(nc.KINDS)
LENS3 = [196, 60, 1]          # 5, 2 and 1 latents
LENS5 = [196, 60, 1, 120, 33]
WINDOW_MAX = 64               # csrc/workspace.h REVERSE_WINDOW_MAX

_DEN, _VAE = {}, {}


def denoiser(kind):
    if kind not in _DEN:
        m = LADiffDenoiser(ABL, **DEN_KW)
        m.load_state_dict(nc.weights(kind), strict=True)
        _DEN[kind] = m.to(DEV).eval()
    _DEN[kind].precision = "fp32"
    return _DEN[kind]


def vae_weights(kind):
    return syn.vae_weights(263) if kind == "plain" else tl.weights("vae", 263, 5)


def vae(kind):
    if kind == "trained":
        return tl.make_vae()
    if kind not in _VAE:
        m = LADiffVae(ABL, **{**VAE_KW, "nfeats": 263})
        m.load_state_dict(vae_weights(kind), strict=True)
        _VAE[kind] = m.to(DEV).eval()
    _VAE[kind].precision = "fp32"
    return _VAE[kind]


# ---------------------------------------------------------------- forward
def run_forward(kind, precision, c, x, txt):
    den = denoiser(kind)
    counts = nc.counts_of(c)
    den.precision = precision
    try:
        got = den(x.to(DEV), torch.tensor(c.timestep), txt.to(DEV), max_iter_elements=None if counts is None else counts.to(DEV))[0]
        torch.cuda.synchronize()
    finally:
        den.precision = "fp32"
    return got


def forward_case(name, kind, precision):
    c = nc.CASES[name]
    (want,), (e32,) = oracle(("ntext", kind, name), nc.forward_fn(c), nc.weights(kind))
    got = run_forward(kind, precision, c, *nc.inputs(c))
    check(f"ntext {c.group} | {name} B={c.B} T={c.T} N={c.N} counts={c.counts} t={c.timestep} {kind}", precision, got, want, e32)
    return c, got


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", nc.names("tokens"))
def test_token_counts(name, kind, precision):
    """B = 4, T = 5, N = 2, 3, 4, 16, 63, 64, 65, 76, 77: the smallest N, the strides of lca_kv_kernel's load loop, the limit."""
    forward_case(name, kind, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", nc.names("latents"))
def test_latent_counts(name, kind, precision):
    """B = 5, T = 1, 2, 7, 8 at N = 2 and 77: the `t < T` guards of the kernels instantiated for TMAX = 8."""
    forward_case(name, kind, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", nc.names("rows"))
def test_row_counts(name, kind, precision):
    """N = 2, M = B T = 1, 31 / 33, 64 / 65, 80 / 81: both sides of the row tiles of the K-resident GEMMs and of gemm_rowln."""
    forward_case(name, kind, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", nc.names("masks"))
def test_masks_and_timesteps(name, kind, precision):
    """B = 6, T = 5, N = 3: counts all T, all 1, mixed and None; the mixed one at timesteps 1, 481 and 981."""
    forward_case(name, kind, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
def test_garbage_in_padded_rows_leaves_the_valid_rows_bits(kind, precision):
    """The mixed-mask case with zeros in the latent rows t >= counts[b] (held to the oracle), then with 1e30 there: no valid row may read
    a padded one, as a key or through a shared reduction.  The 1e30 rows themselves may hold anything."""
    c, clean = forward_case("garbage", kind, precision)
    x, txt = nc.inputs(c, garbage=True)
    dirty = run_forward(kind, precision, c, x, txt)
    valid = orc.count_mask(c.counts, c.T).to(DEV)
    assert (x[~valid.cpu()] == nc.GARBAGE).all() and (~valid).any()
    assert torch.equal(dirty[valid], clean[valid]), (kind, precision, (dirty[valid] - clean[valid]).abs().max().item())


# ---------------------------------------------------------------- unit entry
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("N", [1, 2, 77])
@pytest.mark.parametrize("layer", [0, 4, 8])
def test_linear_cross_attention_unit_entry(layer, N, T, kind):
    """ladiff_linear_cross_attention (fp32 only) against orc.linear_cross_attention with that layer's ca_block parameters; N = 1 runs the
    literal kernels too (the product uses the closed form there)."""
    B = 3
    g = nc.generator(f"lca layer {layer} N {N} T {T}")
    x, xf, emb = torch.randn(B, T, 256, generator=g), torch.randn(B, N, 256, generator=g), torch.randn(B, 256, generator=g)
    counts = nc.mixed_counts(B, T)
    pad = ~orc.count_mask(counts, T)
    (want,), (e32,) = oracle(("ntext-lca", kind, layer, N, T), lambda dt, sd: orc.linear_cross_attention(
        x.to(dt), xf.to(dt), emb.to(dt), nc.block_params(sd, layer), pad), nc.weights(kind))
    L = _lib.lib()
    wt = denoiser(kind)._weight_table()
    xd, xfd, embd = x.to(DEV).contiguous(), xf.to(DEV).contiguous(), emb.to(DEV).contiguous()
    cd = torch.tensor(counts, dtype=torch.int32, device=DEV)
    out = torch.empty_like(xd)
    wsb = L.ladiff_linear_cross_attention_workspace_bytes(B, T, N)
    ws = _lib.workspace(wsb, torch.device(DEV))
    _lib.check(L.ladiff_linear_cross_attention(wt.array, layer, _lib.ptr(xd), _lib.ptr(xfd), _lib.ptr(embd), cd.data_ptr(), B, T, N,
                                               _lib.ptr(out), _lib.ptr(ws), wsb, _lib.stream_ptr()))
    torch.cuda.synchronize()
    check(f"ntext unit | ca_block layer {layer} B={B} T={T} N={N} counts={counts} {kind}", "fp32", out, want, e32)


# ---------------------------------------------------------------- sampling loop
def make_pipe(kind, precision, sched="ddim", steps=5, guidance=7.5, **kw):
    s = (DDIMScheduler(set_alpha_to_one=False, steps_offset=1, **SCHED_KW) if sched == "ddim"
         else DDPMScheduler(variance_type="fixed_small", **SCHED_KW))
    return LADIFF(denoiser=denoiser(kind), vae=vae(kind), scheduler=s, guidance_scale=guidance, num_inference_timesteps=steps, eta=0.0,
                  precision=precision, loop="pipeline", **kw)


def loop_inputs(name, lens, N, guidance):
    g = nc.generator("loop " + name)
    text = torch.randn((2 if guidance > 1.0 else 1) * len(lens), N, 768, generator=g)
    return text, syn.init_noise(lens, seed=zlib.crc32(name.encode()) % 100000)


def loop_case(name, kind, precision, lens, N, guidance=7.5, sched="ddim", steps=5, noise_seed=None, windows=False, **pipe_kw):
    """LADIFF.sample of a text sequence, asked to run as the pipeline kernel: latents and frames against the oracle; the call must have
    completed as launches per stage, rows past a prompt's latent count and frames past its length exactly 0."""
    B = len(lens)
    text, noise = loop_inputs(name, lens, N, guidance)
    pipe = make_pipe(kind, precision, sched, steps, guidance, **pipe_kw)
    pipe.scheduler.set_timesteps(steps)
    n_sched = len(pipe.scheduler.timesteps)
    step_noise = None if noise_seed is None else torch.from_numpy(orc.device_noise(noise_seed, 0, 0, n_sched, B, 5))
    want, e32 = oracle(("ntext-loop", kind, name), lambda dt, den, v: orc.sample_motions(
        den, v, text, lens, noise, steps, sched, guidance_scale=guidance, step_noise=step_noise, dtype=dt), nc.weights(kind), vae_weights(kind))
    if windows:
        pipe.window_ms(enable=True)
    try:
        z, feats = pipe.sample(text.to(DEV), lens, init_noise=noise.to(DEV), noise_seed=noise_seed)
        assert pipe.check()
        assert pipe.loop_status() == (0, 0)
        assert pipe.last_loop()[0] is False          # loop="pipeline" was asked for: a text sequence runs launch per stage
    finally:
        pipe.denoiser.precision = pipe.vae.precision = "fp32"
    assert z.shape == (5, B, 256) and feats.shape == (B, max(lens), 263)
    for i, l in enumerate(lens):
        c = -(-l // 48)
        if c < 5:
            assert z[c:, i].abs().max().item() == 0, (name, i)
        if l < feats.shape[1]:
            assert feats[i, l:].abs().max().item() == 0, (name, i)
    check(f"ntext loop | {name} B={B} N={N} {kind} latents", precision, z, want[0], e32[0])
    check(f"ntext loop | {name} B={B} N={N} {kind} frames", precision, feats, want[1], e32[1], gate=FRAME_TOL)
    return pipe, z, feats, want, e32


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [2, 77])
def test_guided_loop(N, kind, precision):
    """Guided 5-step DDIM, lens 196 / 60 / 1 (5, 2 and 1 latents): the text cache of 2 B N rows, counts[bg % B] in both halves."""
    loop_case(f"guided N={N}", kind, precision, LENS3, N)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
def test_loop_without_guidance(kind, precision):
    """guidance_scale = 1.0: dup = 1, so counts[bg % Bs] indexes the undoubled batch; N = 3."""
    loop_case("no guidance N=3", kind, precision, LENS3, 3, guidance=1.0)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
def test_loop_without_graphs(kind, precision):
    """use_graph=False: no sampler handle, the prologue and every step as plain launches; N = 2."""
    pipe, *_ = loop_case("no graphs N=2", kind, precision, LENS3, 2, use_graph=False)
    assert pipe._sampler is None


@pytest.mark.parametrize("precision", PRECISIONS)
def test_loop_in_chunks(precision):
    """Five prompts with max_prompts_per_launch = 2: three launches (2, 2 and 1 prompts) on two plans, the text rows of each chunk
    gathered from both halves of the duplicated batch; against the oracle and, within the same bound, against the unchunked call."""
    pipe, z, feats, want, e32 = loop_case("chunks N=2", "plain", precision, LENS5, 2, max_prompts_per_launch=2)
    assert [p["key"][0] for p in pipe._last] == [2, 2, 1]
    text, noise = loop_inputs("chunks N=2", LENS5, 2, 7.5)
    whole = make_pipe("plain", precision, max_prompts_per_launch=None)
    try:
        z1, feats1 = whole.sample(text.to(DEV), LENS5, init_noise=noise.to(DEV))
    finally:
        whole.denoiser.precision = whole.vae.precision = "fp32"
    assert [p["key"][0] for p in whole._last] == [5]
    check("ntext loop | chunks N=2 latents against the unchunked call", precision, z, z1.double().cpu(), e32[0])
    check("ntext loop | chunks N=2 frames against the unchunked call", precision, feats, feats1.double().cpu(), e32[1], gate=FRAME_TOL)


def smallest_long_schedule():
    """The smallest num_inference_timesteps whose DDPM schedule has more than WINDOW_MAX positions (the schedule's length is
    ceil(1000 / (1000 // n)), not n)."""
    sch = DDPMScheduler(variance_type="fixed_small", **SCHED_KW)
    for n in range(1, 1001):
        sch.set_timesteps(n)
        if len(sch.timesteps) > WINDOW_MAX:
            return n, len(sch.timesteps)
    raise AssertionError("no schedule longer than a window")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ddpm_loop_over_more_than_one_window(precision):
    """DDPM, B = 2, N = 2, the shortest schedule of more than 64 positions: at least two windows of steps, none of which builds a c table
    for this route.  The noise is drawn on the device from `noise_seed`; the oracle is fed orc.device_noise of that seed.  Plain weights
    only (the module's docstring says why)."""
    steps, n_sched = smallest_long_schedule()
    seed = 0x5EED0000 + steps
    pipe, *_ = loop_case(f"ddpm {steps} N=2", "plain", precision, [196, 60], 2, sched="ddpm", steps=steps, noise_seed=seed, windows=True)
    plan = pipe._plan
    assert plan["n"] == n_sched and plan["n"] > WINDOW_MAX and plan["need_noise"] and pipe.last_noise_seed == seed
    windows = pipe.window_ms()[1]
    assert windows >= 2 and plan["n"] % windows == 0, (plan["n"], windows)
    print(f"\n[ntext loop] DDPM num_inference_timesteps {steps}: {plan['n']} positions in {windows} windows of {plan['n'] // windows}")


# ---------------------------------------------------------------- refusals
def test_more_than_77_tokens_are_refused():
    """N = 78 (> LADIFF_CLIP_MAX_POSITIONS) through the forward and through the loop: LadiffHipError, and the same N = 2 call gives the
    same bits before and after."""
    c = nc.CASES["tokens2"]
    x, txt = nc.inputs(c)
    before = run_forward("plain", "fp32", c, x, txt)
    with pytest.raises(_lib.LadiffHipError):
        denoiser("plain")(x.to(DEV), torch.tensor(c.timestep), torch.randn(c.B, 78, 768).to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(run_forward("plain", "fp32", c, x, txt), before)

    text, noise = loop_inputs("guided N=2", LENS3, 2, 7.5)
    pipe = make_pipe("plain", "fp32")
    try:
        z0, f0 = pipe.sample(text.to(DEV), LENS3, init_noise=noise.to(DEV))
        with pytest.raises(_lib.LadiffHipError):
            pipe.sample(torch.randn(6, 78, 768).to(DEV), LENS3, init_noise=noise.to(DEV))
        torch.cuda.synchronize()
        z1, f1 = pipe.sample(text.to(DEV), LENS3, init_noise=noise.to(DEV))
    finally:
        pipe.denoiser.precision = pipe.vae.precision = "fp32"
    assert torch.equal(z0, z1) and torch.equal(f0, f1)


def test_edit_and_per_sample_timesteps_refuse_a_text_sequence():
    """An edit with N = 2 and per-sample timesteps with N = 2: NotImplementedError on the host, nothing launched."""
    text, noise = loop_inputs("guided N=2", LENS3, 2, 7.5)
    pipe = make_pipe("plain", "fp32")
    try:
        with pytest.raises(NotImplementedError):
            pipe.sample(text.to(DEV), LENS3, init_noise=noise.to(DEV), source_latents=torch.zeros(5, 3, 256, device=DEV), strength=0.5)
    finally:
        pipe.denoiser.precision = pipe.vae.precision = "fp32"
    assert pipe._plan is None and not pipe._pending
    c = nc.CASES["tokens2"]
    x, txt = nc.inputs(c)
    with pytest.raises(NotImplementedError):
        denoiser("plain")(x.to(DEV), torch.tensor([1, 481, 981, 481]), txt.to(DEV))
