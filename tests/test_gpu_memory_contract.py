"""Every workspace-taking entry of the C ABI (and the strided GEMM entries) held to its memory contract, tests/memory_contract.py: the
workspace and every output sit inside guard zones and are filled - guards included - with zero, a quiet NaN and +inf in turn.  A result
may not depend on the fill, no guard or gap word may change, a workspace 4 bytes short of the query is refused on the host with the
outputs untouched, and one 1 MiB larger gives the same contract.  `want` comes from the CPU oracle (or a golden captured from the
reference) and every tolerance from the existing parity test of the same entry, named at each case.

Safety: an overrun lands in memory this file owns (the guards); no entry is ever LAUNCHED on a workspace below its query (the short case
is refused by host code); a sampler's workspace is poisoned only before the first call of a FRESH sampler, never between two calls of one
handle (the pipeline's stage table lives there, include/ladiff_hip.h); every configuration runs once."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from ladiff_amd import DDIMScheduler, DDPMScheduler, LADiffDenoiser, LADiffVae, _lib, synthetic as syn
from ladiff_amd.schedulers import timestep_sinusoid
from ladiff_amd.schema import ABL, DEN_KW, VAE_KW
from oracle import ladiff_oracle as orc
from conftest import load_golden
from memory_contract import FILLS, Out, assert_contract, assert_refused, run_fills, run_in_guards

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIB = 1 << 20
SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False)


def L():
    return _lib.lib()


def st():
    return _lib.stream_ptr()


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (scale * torch.randn(*shape, generator=g)).float()


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def ints(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def hold(what, call, ws_bytes, outs, want, tol):
    """The whole contract of one configuration: refused 4 bytes short (workspace-taking entries), exact size, 1 MiB larger."""
    if ws_bytes:
        assert_refused(run_in_guards(call, ws_bytes - 4, outs, FILLS["nan"]), what + ", workspace 4 bytes short")
    rep = assert_contract(run_fills(call, ws_bytes, outs), want, tol, what)
    if ws_bytes:
        big = assert_contract(run_fills(call, ws_bytes, outs, ws_extra_bytes=MIB), want, tol, what + ", workspace 1 MiB larger")
        rep["identical"] = rep["identical"] and big["identical"]
        rep["guards"], rep["gaps"] = rep["guards"] + big["guards"], rep["gaps"] + big["gaps"]
    report(what, rep)
    return rep


def report(what, rep):
    """One line per configuration, every figure measured (assert_contract's report)."""
    print(f"memory contract | {what}: guard words touched {rep['guards']}, gap words touched {rep['gaps']}, "
          f"fills bit-identical: {rep['identical']}, deterministic: {rep['deterministic']}")


def split_rows(t):
    s = torch.empty_like(t)
    _lib.check(L().ladiff_split_rows(_lib.ptr(t), _lib.ptr(s), t.shape[0], t.shape[1], st()))
    return s


def from_split(y):
    """S-format words [R, K] (int32, CPU) -> fp32 hi + lo."""
    half = torch.float16 if L().ladiff_split_format() == 1 else torch.bfloat16
    b = y.contiguous().view(half).view(y.shape[0], y.shape[1] // 64, 2, 64).float()
    return (b[:, :, 0] + b[:, :, 1]).reshape(y.shape[0], y.shape[1])


def ref_gemm(A, W, bias=None, res=None, ln=None):
    y = F.linear(A.double(), W.double(), None if bias is None else bias.double())
    if res is not None:
        y = y + res.double()
    if ln is not None:
        y = F.layer_norm(y, (y.shape[-1],), ln[0].double(), ln[1].double(), 1e-5)
    return y


# ---------------------------------------------------------------- networks (synthetic weights), built once per module
@pytest.fixture(scope="module")
def denoiser():
    m = LADiffDenoiser(ABL, **DEN_KW)
    m.load_state_dict(syn.denoiser_weights(), strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def vaes():
    out = {}
    for C in (263, 251):
        m = LADiffVae(ABL, **{**VAE_KW, "nfeats": C})
        m.load_state_dict(syn.vae_weights(C), strict=True)
        out[C] = m.to(DEV).eval()
    return out


def tables_of(module, precision, kind=None):
    wt = module._weight_table(kind) if kind else module._weight_table()
    return wt, (wt.split_array() if precision == "f16x3" else None)


# ---------------------------------------------------------------- strided GEMM entries: outputs and gaps (no workspace)
@pytest.mark.parametrize("form", ["bias_res", "layernorm"])
def test_gemm_strided(form):
    """ladiff_gemm with lda / ldres / ldy wider than the rows.  Tolerances: test_gpu_kernels.py::test_gemm_bias_act (2e-5 x max(1, |want|))
    and ::test_gemm_residual_layernorm (2e-5)."""
    M, K = 33, 256
    N, ldy = (263, 272) if form == "bias_res" else (256, 320)
    lda, ldres = 288, 264
    A, W, b, res = rnd(M, lda), rnd(N, K, scale=1 / 16), rnd(N), rnd(M, ldres, seed=5)
    ln = (1 + 0.1 * rnd(256, seed=3), 0.1 * rnd(256, seed=4)) if form == "layernorm" else None
    want = ref_gemm(A[:, :K], W, b, res[:, :N], ln)
    Ad, Wd, bd, rd = dev(A), dev(W), dev(b), dev(res)
    g, be = (dev(ln[0]), dev(ln[1])) if ln else (None, None)

    def call(ws, wsb, o):
        return L().ladiff_gemm(_lib.ptr(Ad), lda, None, 0, K, _lib.ptr(Wd), K, _lib.ptr(bd), _lib.ptr(rd), ldres, _lib.ptr(g), _lib.ptr(be),
                               o["Y"], ldy, M, N, K, 0, st())
    hold(f"ladiff_gemm {form} ({M},{N},{K}) ldy {ldy}", call, 0, {"Y": Out(M, N, ldy)}, {"Y": want},
         2e-5 * max(1.0, want.abs().max().item()) if ln is None else 2e-5)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("K", [256, 1024])
def test_gemm_resident_strided(K, split):
    """ladiff_gemm_resident, M = 45, N = 256, ldy = 320: K = 256 with bias + residual (and the S-format twin in split mode), K = 1024 as
    four raw planes [4][M][ldy].  Tolerances: test_gpu_kernels.py::test_gemm_resident_k256 (2e-5 x max(1, |want|)),
    ::test_gemm_resident_split_k_and_combine (plane sum 2e-5), ::test_gemm_resident_split (4 x 2^-16 x max |A||W|^T; Ys within 2^-15 |Y|)."""
    M, N, ldy = 45, 256, 320
    A, W, b, res = rnd(M, K, scale=2.0), rnd(N, K, scale=1 / math.sqrt(K)), rnd(N), rnd(M, N, seed=7)
    Ad, Wd, bd, rd = dev(A), dev(W), dev(b), dev(res)
    if split:
        Ad, Wd = split_rows(Ad), split_rows(Wd)
    planes = K // 256
    outs = {"Y": Out(planes * M, N, ldy)}
    if split and planes == 1:
        outs["Ys"] = Out(M, N, ldy, dtype=torch.int32)
    single = planes == 1

    def call(ws, wsb, o):
        return L().ladiff_gemm_resident(_lib.ptr(Ad), K, None, 0, K, _lib.ptr(Wd), K, _lib.ptr(bd) if single else None,
                                        _lib.ptr(rd) if single else None, N, o["Y"], ldy, M, N, K, 0, split, o.get("Ys"), st())
    want = ref_gemm(A, W, b, res) if single else ref_gemm(A, W)
    mag = (A.abs().double() @ W.abs().double().t()).max().item()
    tol = 4 * 2.0 ** -16 * mag if split else (2e-5 * max(1.0, want.abs().max().item()) if single else 2e-5)
    res_ = run_fills(call, 0, outs)
    if single:
        rep = assert_contract(res_, {"Y": want}, tol, f"ladiff_gemm_resident K {K} split {split}")
        if split:
            y = res_["nan"]["outputs"]["Y"]
            assert (from_split(res_["nan"]["outputs"]["Ys"]).double() - y.double()).abs().max().item() <= 2.0 ** -15 * y.abs().max().item()
    else:
        rep = assert_contract(res_, {}, tol, f"ladiff_gemm_resident K {K} split {split}")
        got = res_["nan"]["outputs"]["Y"].view(planes, M, N).double().sum(0)
        assert (got - want).abs().max().item() < tol
    report(f"ladiff_gemm_resident K {K} split {split}", rep)


def test_gemm_split_strided():
    """ladiff_gemm_split M = 130, N = 128, K = 64, ldy = 192, fp32 and S-format outputs.  Tolerance: test_gpu_kernels.py::
    test_gemm_split_large_m (4 x 2^-16 x max |A||W|^T + 2e-6; Ys within 2^-15 |Y|)."""
    M, N, K, ldy = 130, 128, 64, 192
    A, W, b = rnd(M, K, scale=2.0), rnd(N, K, scale=1 / math.sqrt(K)), rnd(N)
    As, Ws, bd = split_rows(dev(A)), split_rows(dev(W)), dev(b)

    def call(ws, wsb, o):
        return L().ladiff_gemm_split(_lib.ptr(As), K, None, 0, K, _lib.ptr(Ws), K, _lib.ptr(bd), None, 0, o["Y"], o["Ys"], ldy, M, N, K, 0, st())
    want = ref_gemm(A, W, b)
    tol = 4 * 2.0 ** -16 * (A.abs().double() @ W.abs().double().t()).max().item() + 2e-6
    res = run_fills(call, 0, {"Y": Out(M, N, ldy), "Ys": Out(M, N, ldy, dtype=torch.int32)})
    rep = assert_contract(res, {"Y": want}, tol, "ladiff_gemm_split")
    y = res["inf"]["outputs"]["Y"]
    assert (from_split(res["inf"]["outputs"]["Ys"]).double() - y.double()).abs().max().item() <= 2.0 ** -15 * y.abs().max().item()
    report("ladiff_gemm_split", rep)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_mlp_ln_fused_pad_rows(variant):
    """ladiff_mlp_ln_fused at M = 17 (one row past a 16-row wave tile), y and ys, every launch variant.  Tolerance: test_gpu_kernels.py::
    test_fused_mlp_layernorm (2e-4; ys within 1e-4 of y)."""
    M = 17
    x = rnd(M, 256, scale=2.0, seed=1)
    w1, b1 = rnd(1024, 256, scale=1 / 16, seed=2), rnd(1024, scale=0.5, seed=3)
    w2, b2 = rnd(256, 1024, scale=1 / 32, seed=4), rnd(256, scale=0.5, seed=5)
    g3, be3, g4, be4 = 1 + 0.1 * rnd(256, seed=6), 0.1 * rnd(256, seed=7), 1 + 0.1 * rnd(256, seed=8), 0.1 * rnd(256, seed=9)
    xd = dev(x)
    xs, w1s, w2s = split_rows(xd), split_rows(dev(w1)), split_rows(dev(w2))
    b1d, b2d, g3d, be3d, g4d, be4d = dev(b1), dev(b2), dev(g3), dev(be3), dev(g4), dev(be4)

    def call(ws, wsb, o):
        return L().ladiff_mlp_ln_fused(_lib.ptr(xs), _lib.ptr(xd), _lib.ptr(w1s), _lib.ptr(b1d), _lib.ptr(w2s), _lib.ptr(b2d), _lib.ptr(g3d),
                                       _lib.ptr(be3d), _lib.ptr(g4d), _lib.ptr(be4d), o["y"], o["ys"], M, st())
    h = F.gelu(F.linear(x.double(), w1.double(), b1.double()))
    want = F.layer_norm(x.double() + F.linear(h, w2.double(), b2.double()), (256,), g3.double(), be3.double(), 1e-5)
    want = F.layer_norm(want, (256,), g4.double(), be4.double(), 1e-5)
    assert L().ladiff_debug_set_mlp_variant(variant) == 0
    try:
        res = run_fills(call, 0, {"y": Out(M, 256), "ys": Out(M, 256, dtype=torch.int32)})
    finally:
        L().ladiff_debug_set_mlp_variant(0)
    rep = assert_contract(res, {"y": want}, 2e-4, f"ladiff_mlp_ln_fused variant {variant}")
    assert (from_split(res["nan"]["outputs"]["ys"]).double() - res["nan"]["outputs"]["y"].double()).abs().max().item() < 1e-4
    report(f"ladiff_mlp_ln_fused variant {variant}", rep)


# ---------------------------------------------------------------- denoiser: time tables -> text cache -> forward, one workspace
@pytest.mark.parametrize("Bs,T,n_text,precision", [(7, 3, 1, "fp32"), (7, 3, 1, "f16x3"), (33, 5, 1, "fp32"), (33, 5, 1, "f16x3"),
                                                   (7, 3, 4, "fp32")])
def test_denoiser_chain(denoiser, Bs, T, n_text, precision):
    """dup = 2, mixed latent counts: (B2, T) = (14, 3) and (66, 5) = 330 rows (not a multiple of 16).  The workspace is poisoned once,
    before the chain; `tables` and the text cache are caller buffers later calls read, so they are outputs here.  Tolerance:
    test_gpu_path.py::test_denoiser_split_shapes_against_oracle (fp32 5e-5, f16x3 1e-3 against the CPU oracle)."""
    B2, t = 2 * Bs, 301
    gen = torch.Generator().manual_seed(100 * Bs + T + n_text)
    x = torch.randn(Bs, T, 256, generator=gen)
    text = torch.randn(B2, n_text, 768, generator=gen)
    counts = torch.randint(1, T + 1, (Bs,), generator=gen)
    want = orc.denoiser_forward(syn.denoiser_weights(), torch.cat([x, x]), t, text, torch.cat([counts, counts]))
    wt, wsplit = tables_of(denoiser, precision)
    xd, textd, cd = dev(x), dev(text), ints(counts.tolist())
    sinus = timestep_sinusoid(torch.tensor([t]), 768).to(DEV)
    step0 = torch.zeros(4, dtype=torch.int32, device=DEV)
    n_tab, n_cache = L().ladiff_denoiser_tables_floats(1), L().ladiff_denoiser_text_cache_floats(B2, 1, n_text)
    wsb = L().ladiff_denoiser_workspace_bytes(B2, T, 1, n_text)
    outs = {"tables": Out(1, n_tab), "cache": Out(1, n_cache), "eps": Out(B2 * T, 256)}

    def call(ws, nbytes, o):
        rc = L().ladiff_denoiser_time_tables(wt.array, _lib.ptr(sinus), 1, o["tables"], ws, nbytes, st())
        rc = rc or L().ladiff_denoiser_text_cache(wt.array, _lib.ptr(textd), B2, n_text, o["tables"], 1, o["cache"], ws, nbytes, st())
        return rc or L().ladiff_denoiser_forward(wt.array, wsplit, o["tables"], step0.data_ptr(), o["cache"], n_text, 1, _lib.ptr(xd), Bs, 2, T,
                                                 cd.data_ptr(), o["eps"], ws, nbytes, st())
    what = f"denoiser chain B2 {B2} T {T} n_text {n_text} {precision}"
    # each entry by itself refuses a workspace below the query at ITS arguments (the ones it does not take at 1: include/ladiff_hip.h)
    q_tab, q_txt = L().ladiff_denoiser_workspace_bytes(1, 1, 1, 1), L().ladiff_denoiser_workspace_bytes(B2, 1, 1, n_text)
    short = lambda fn, q: assert_refused(run_in_guards(fn, q - 4, outs, FILLS["nan"]), what + ", single entry 4 bytes short")
    short(lambda ws, nb, o: L().ladiff_denoiser_time_tables(wt.array, _lib.ptr(sinus), 1, o["tables"], ws, nb, st()), q_tab)
    short(lambda ws, nb, o: L().ladiff_denoiser_text_cache(wt.array, _lib.ptr(textd), B2, n_text, o["tables"], 1, o["cache"], ws, nb, st()), q_txt)
    short(lambda ws, nb, o: L().ladiff_denoiser_forward(wt.array, wsplit, o["tables"], step0.data_ptr(), o["cache"], n_text, 1, _lib.ptr(xd), Bs,
                                                        2, T, cd.data_ptr(), o["eps"], ws, nb, st()), wsb)
    rep = assert_contract(run_fills(call, wsb, outs), {"eps": want}, 5e-5 if precision == "fp32" else 1e-3, what)
    big = assert_contract(run_fills(call, wsb, outs, ws_extra_bytes=MIB), {"eps": want}, 5e-5 if precision == "fp32" else 1e-3, what + ", 1 MiB larger")
    rep["identical"] = rep["identical"] and big["identical"]
    rep["guards"], rep["gaps"] = rep["guards"] + big["guards"], rep["gaps"] + big["gaps"]
    report(what, rep)


def test_linear_cross_attention(denoiser):
    """golden cross_attention_n4 (B 3, T 5, N 4).  Tolerance: test_gpu_path.py::test_linear_cross_attention_general_n_golden (2e-5)."""
    g = load_golden("cross_attention_n4")
    B, T, N = 3, 5, 4
    wt = denoiser._weight_table()
    x, xf, emb = dev(g["x"]), dev(g["xf"]), dev(g["emb"])
    counts = (~g["pad"]).sum(1).to(torch.int32).to(DEV)

    def call(ws, nb, o):
        return L().ladiff_linear_cross_attention(wt.array, 0, _lib.ptr(x), _lib.ptr(xf), _lib.ptr(emb), counts.data_ptr(), B, T, N, o["out"], ws, nb, st())
    hold("ladiff_linear_cross_attention N 4", call, L().ladiff_linear_cross_attention_workspace_bytes(B, T, N), {"out": Out(B * T, 256)},
         {"out": g["out"]}, 2e-5)


# ---------------------------------------------------------------- reverse loop
REV_LENS = [60, 120, 196, 24, 60, 120, 196]


class _DDPMExact(orc.DDPM):
    """orc.DDPM whose schedule has EXACTLY n steps (arange(0, 1000, 1000 // 70) has 72): the n smallest timesteps.  With prev_timestep
    "t-1" a step's coefficients depend on its own t only, so any subset of timesteps is a valid schedule."""

    def set_timesteps(self, n):
        super().set_timesteps(n)
        self.timesteps = self.timesteps[-n:]


_REV_CACHE = {}


def reverse_case(sched, n, lens, seed):
    """Inputs, tables and the oracle's z for one reverse loop; computed once and shared by the arithmetic modes and loop forms."""
    key = (sched, n, tuple(lens), seed)
    if key not in _REV_CACHE:
        B = len(lens)
        text, noise = syn.text_embeddings(B, seed=seed), syn.init_noise(lens, seed=seed + 1)
        if sched == "ddim":
            s = DDIMScheduler(set_alpha_to_one=False, steps_offset=1, **SCHED_KW)
            s.set_timesteps(n)
            osch, step_noise = orc.DDIM(), None
        else:
            s = DDPMScheduler(variance_type="fixed_small", **SCHED_KW)
            s.set_timesteps(n)
            s.timesteps = s.timesteps[-n:]
            osch = _DDPMExact()
            step_noise = torch.from_numpy(orc.device_noise(seed, 0, 0, n, B, 5))      # what the device generator draws for this seed
        assert len(s.timesteps) == n
        sd = syn.denoiser_weights()
        with torch.no_grad():
            z = orc.diffusion_reverse(lambda x, t, txt, c: orc.denoiser_forward(sd, x, t, txt, c), osch, text, lens, noise, n, 7.5, 0.0,
                                      step_noise)
        assert torch.equal(osch.timesteps, s.timesteps)
        _REV_CACHE[key] = dict(text=dev(text), noise=dev(noise), coef=dev(s.coef_table(0.0)), sinus=dev(timestep_sinusoid(s.timesteps, 768)),
                               z=z, counts=syn.max_iter_elements(lens))
    return _REV_CACHE[key]


def reverse_call(denoiser, precision, c, B, T, n, sampler_loop=None, seed=0, stream=None, statuses=None):
    """call(ws, ws_bytes, outs) for ladiff_diffusion_reverse.  sampler_loop None: sampler == NULL (the workspace is pure scratch).
    Otherwise every run makes a FRESH sampler (set_loop `sampler_loop`), calls once, reads the status words and which loop form ran
    (`statuses` gets (status code, 1 = pipeline kernel / 0 = launch-per-stage graphs)) and destroys the handle: the poison is in place
    before the first - and only - call of that sampler."""
    wt, wsplit = tables_of(denoiser, precision)
    cd = ints(c["counts"])
    h_counts = (ctypes.c_int32 * B)(*c["counts"])

    def one(sampler, ws, nb, o, s):
        return L().ladiff_diffusion_reverse(sampler, wt.array, wsplit, wt.generation, _lib.ptr(c["text"]), _lib.ptr(c["noise"]), cd.data_ptr(),
                                            cd.data_ptr(), h_counts, _lib.ptr(c["sinus"]), _lib.ptr(c["coef"]), None, 7.5, 1.0, 1, B, T, 1, n,
                                            o["z"], ws, nb, 0, s)

    def call(ws, nb, o):
        if sampler_loop is None:
            return one(None, ws, nb, o, st())
        h = ctypes.c_void_p()
        _lib.check(L().ladiff_sampler_create(ctypes.byref(h)))
        try:
            _lib.check(L().ladiff_sampler_set_loop(h, sampler_loop))
            _lib.check(L().ladiff_sampler_set_noise_generator(h, seed, 0, 1 if seed else 0))
            rc = one(h, ws, nb, o, stream.cuda_stream)              # a real stream: the handle replays its graphs on it
            stream.synchronize()
            if rc == 0:
                code, info = ctypes.c_int(-1), ctypes.c_int(0)
                _lib.check(L().ladiff_reverse_status(ws, B, T, n, 1, ctypes.byref(code), ctypes.byref(info)))
                piped = ctypes.c_int(-1)                            # did the persistent pipeline kernel run, or launch-per-stage graphs?
                _lib.check(L().ladiff_sampler_last_loop(h, ctypes.byref(piped), None, None))
                statuses.append((code.value, piped.value))
        finally:
            _lib.check(L().ladiff_sampler_destroy(h))
        return rc
    return call


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_reverse_without_sampler(denoiser, precision):
    """sampler == NULL, B = 7, T = 5, cfg 1, 5-step DDIM.  Tolerance: test_gpu_path.py::test_sampling_loop_many_text_tokens (z against
    the CPU oracle: fp32 2e-5, f16x3 5e-4, x max(1, |z|))."""
    B, T, n = len(REV_LENS), 5, 5
    c = reverse_case("ddim", n, REV_LENS, 141)
    scale = max(1.0, c["z"].abs().max().item())
    hold(f"ladiff_diffusion_reverse sampler NULL {precision}", reverse_call(denoiser, precision, c, B, T, n),
         L().ladiff_reverse_workspace_bytes(B, T, n, 1), {"z": Out(T * B, 256)}, {"z": c["z"]}, (2e-5 if precision == "fp32" else 5e-4) * scale)


@pytest.mark.parametrize("loop", [0, 2, 3])
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_reverse_with_fresh_sampler(denoiser, precision, loop):
    """A fresh sampler per run, launch-per-stage graphs (0) and the pipeline kernel with 16- (2) and 32-row (3) blocks; the status must
    read "completed".  Tolerance as test_reverse_without_sampler."""
    B, T, n = len(REV_LENS), 5, 5
    c = reverse_case("ddim", n, REV_LENS, 141)
    scale = max(1.0, c["z"].abs().max().item())
    statuses, stream = [], torch.cuda.Stream()
    hold(f"ladiff_diffusion_reverse fresh sampler loop {loop} {precision}",
         reverse_call(denoiser, precision, c, B, T, n, loop, stream=stream, statuses=statuses),
         L().ladiff_reverse_workspace_bytes(B, T, n, 1), {"z": Out(T * B, 256)}, {"z": c["z"]}, (2e-5 if precision == "fp32" else 5e-4) * scale)
    # completed, and by the loop form asked for: a silent fall-back to the step graphs would leave the stage table and the hand-off slots untested
    assert statuses and all(s == (0, int(loop != 0)) for s in statuses), statuses


@pytest.mark.parametrize("loop", [0, 2, 3])
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_reverse_with_fresh_sampler_70_step_ddpm(denoiser, precision, loop):
    """B = 3, 70-step DDPM with the device noise generator: more than 64 steps run as several windows (7 of 10 steps) and the hoisted
    cross-attention table is rebuilt inside the workspace before each.  Tolerance: the DDPM cases against the oracle,
    test_gpu_path.py::test_ddpm_1000_steps_small_batch (fp32 1e-4 x max(1, |z|)) and ::test_ddpm_1000_steps_full_batch_properties (f16x3 2e-3)."""
    lens, T, n, seed = [196, 60, 120], 5, 70, 977
    B = len(lens)
    c = reverse_case("ddpm", n, lens, seed)
    scale = max(1.0, c["z"].abs().max().item())
    statuses, stream = [], torch.cuda.Stream()
    hold(f"ladiff_diffusion_reverse fresh sampler loop {loop} 70-step DDPM {precision}",
         reverse_call(denoiser, precision, c, B, T, n, loop, seed=seed, stream=stream, statuses=statuses),
         L().ladiff_reverse_workspace_bytes(B, T, n, 1), {"z": Out(T * B, 256)}, {"z": c["z"]}, (1e-4 if precision == "fp32" else 2e-3) * scale)
    # completed, and by the loop form asked for: a silent fall-back to the step graphs would leave the stage table and the hand-off slots untested
    assert statuses and all(s == (0, int(loop != 0)) for s in statuses), statuses


@pytest.mark.parametrize("loop", [0, 2, 3])
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("n", [65, 67])
def test_reverse_with_fresh_sampler_odd_windows(denoiser, precision, loop, n):
    """B = 3, DDPM schedules above 64 steps that have no divisor that is a multiple of 10 (csrc/workspace.h reverse_window): 65 steps run as 5
    windows of 13 and the prime 67 as 67 windows of 1 - odd windows, step graphs that hold one step, the c table rebuilt for 13 steps or
    one, the pipeline kernel relaunched at an odd first step - inside a workspace that reserves 64 steps of table.  Tolerance as
    test_reverse_with_fresh_sampler_70_step_ddpm."""
    lens, T, seed = [196, 60, 120], 5, 977
    B = len(lens)
    c = reverse_case("ddpm", n, lens, seed)
    scale = max(1.0, c["z"].abs().max().item())
    statuses, stream = [], torch.cuda.Stream()
    hold(f"ladiff_diffusion_reverse fresh sampler loop {loop} {n}-step DDPM {precision}",
         reverse_call(denoiser, precision, c, B, T, n, loop, seed=seed, stream=stream, statuses=statuses),
         L().ladiff_reverse_workspace_bytes(B, T, n, 1), {"z": Out(T * B, 256)}, {"z": c["z"]}, (1e-4 if precision == "fp32" else 2e-3) * scale)
    assert statuses and all(s == (0, int(loop != 0)) for s in statuses), statuses


# ---------------------------------------------------------------- LA-VAE decoder and encoder
_DEC_CACHE = {}


def decode_case(name):
    if name not in _DEC_CACHE:
        if name == "golden":                                   # lengths [37, 49, 5, 101]: the small-M routing
            g = load_golden("vae_decode_ragged")
            _DEC_CACHE[name] = (g["lengths"].tolist(), g["z"], g["feats"], 1)
        else:                                                  # 4145 frame rows, every fused decoder kernel (dec_mlp, dec_qkv_attn, dec_out_cross)
            lens = [196] * 20 + [224, 1]
            z = torch.randn(5, len(lens), 256, generator=torch.Generator().manual_seed(4))
            for i, l in enumerate(lens):
                z[-(-l // 48):, i] = 0
            with torch.no_grad():
                _DEC_CACHE[name] = (lens, z, orc.vae_decode(syn.vae_weights(263), z, lens), 2)
    return _DEC_CACHE[name]


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", ["golden", "fused_4145_rows"])
def test_vae_decode(vaes, name, precision, ragged):
    """ladiff_vae_decode and ladiff_vae_decode_ragged.  Tolerances: test_gpu_path.py::test_vae_decode_golden (fp32 1e-4) and
    ::test_vae_decode_golden_split (f16x3: half the 1e-3 frame gate)."""
    lens, z, want, fusion = decode_case(name)
    B, Fr, T, C = len(lens), max(lens), 5, 263
    wt, wsplit = tables_of(vaes[C], precision)
    zd, ld, cd = dev(z), ints(lens), ints(syn.max_iter_elements(lens))
    off = [0]
    for l in lens:
        off.append(off[-1] + l)
    od = ints(off)

    def call(ws, nb, o):
        if ragged:
            return L().ladiff_vae_decode_ragged(wt.array, wsplit, _lib.ptr(zd), ld.data_ptr(), cd.data_ptr(), od.data_ptr(), off[-1], B, Fr, T, C,
                                                o["feats"], ws, nb, st())
        return L().ladiff_vae_decode(wt.array, wsplit, _lib.ptr(zd), ld.data_ptr(), cd.data_ptr(), B, Fr, T, C, o["feats"], ws, nb, st())
    assert L().ladiff_debug_set_decoder_fusion(fusion) == 0
    try:
        hold(f"ladiff_vae_decode{'_ragged' if ragged else ''} {name} {precision}", call, L().ladiff_decoder_workspace_bytes(B, Fr, T, C),
             {"feats": Out(B * Fr, C)}, {"feats": want}, 1e-4 if precision == "fp32" else 5e-4)
    finally:
        L().ladiff_debug_set_decoder_fusion(1)


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("C", [263, 251])
def test_vae_encode(vaes, C, precision):
    """B = 3, lengths [37, 101, 5], T = 5.  Tolerance: test_gpu_path.py::test_vae_encode_golden (fp32 1e-4, f16x3 2e-3; std and latent
    relative to max(1, their size))."""
    lens, T = [37, 101, 5], 5
    B, Fr = len(lens), max(lens)
    gen = torch.Generator().manual_seed(C)
    feats, eps = torch.randn(B, Fr, C, generator=gen), torch.randn(T, B, 256, generator=gen)
    with torch.no_grad():
        mu, sd, lat = orc.vae_encode(syn.vae_weights(C), feats, lens, eps)
    wt, wsplit = tables_of(vaes[C], precision, "encoder")
    fd, ed, ld, cd = dev(feats), dev(eps), ints(lens), ints(syn.max_iter_elements(lens))

    def call(ws, nb, o):
        return L().ladiff_vae_encode(wt.array, wsplit, _lib.ptr(fd), ld.data_ptr(), cd.data_ptr(), _lib.ptr(ed), B, Fr, T, C, o["mu"], o["std"],
                                     o["latent"], ws, nb, st())
    tol = 1e-4 if precision == "fp32" else 2e-3
    hold(f"ladiff_vae_encode C {C} {precision}", call, L().ladiff_encoder_workspace_bytes(B, Fr, T, C),
         {k: Out(T * B, 256) for k in ("mu", "std", "latent")}, {"mu": mu, "std": sd, "latent": lat},
         {"mu": tol, "std": tol * max(1.0, sd.max().item()), "latent": tol * max(1.0, lat.abs().max().item())})


# ---------------------------------------------------------------- CLIP text tower
def clip_ids(seq_lens, vocab, S=77, seed=3):
    """[BOS, words, EOS, EOS padding]: prompt b has seq_lens[b] positions up to and including its EOS."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(seq_lens), S), vocab - 1, dtype=torch.int64)
    ids[:, 0] = vocab - 2
    for b, n in enumerate(seq_lens):
        ids[b, 1:n - 1] = torch.randint(0, vocab - 2, (n - 2,), generator=g)
    return ids


@pytest.fixture(scope="module")
def clip_tower():
    from ladiff_amd.text_encoder import MldTextEncoder
    m = MldTextEncoder(vocab_size=512, num_layers=2)
    m.text_model.load_state_dict(syn.clip_weights(512, 2), strict=True)
    return m.to(DEV).eval()


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("rows", ["padded_256", 255, 256, 257])
def test_clip_text_encode(clip_tower, rows, precision):
    """vocab 512, 2 layers, 8 prompts; total rows 255 / 256 / 257 straddle the small-row regime of clip_plane_floats (the padded form:
    B = 8, L = 32 = 256 rows).  Tolerance: test_gpu_clip.py TOL (fp32 5e-5, f16x3 5e-4 against the CPU oracle)."""
    vocab, layers, S = 512, 2, 77
    seq = {"padded_256": [32] * 7 + [31], 255: [32] * 7 + [31], 256: [32] * 8, 257: [33] + [32] * 7}[rows]
    B, Lx = len(seq), max(seq)
    ids = clip_ids(seq, vocab)
    with torch.no_grad():
        want = orc.clip_text_features(syn.clip_weights(vocab, layers), ids, layers)
    wt, wsplit = tables_of(clip_tower.text_model, precision)
    idd = ids.to(DEV)
    off = [0]
    for n in seq:
        off.append(off[-1] + n)
    sl, od, rs = ints(seq), ints(off), ints([b for b, n in enumerate(seq) for _ in range(n)])
    if rows == "padded_256":
        wsb = L().ladiff_clip_workspace_bytes(B, Lx)
        call = lambda ws, nb, o: L().ladiff_clip_text_encode(wt.array, wsplit, layers, vocab, idd.data_ptr(), B, S, Lx, o["out"], ws, nb, st())
    else:
        assert off[-1] == rows
        wsb = L().ladiff_clip_workspace_bytes_ragged(B, rows)
        call = lambda ws, nb, o: L().ladiff_clip_text_encode_ragged(wt.array, wsplit, layers, vocab, idd.data_ptr(), B, S, Lx, sl.data_ptr(),
                                                                      od.data_ptr(), rs.data_ptr(), rows, o["out"], ws, nb, st())
    hold(f"ladiff_clip_text_encode{'' if rows == 'padded_256' else '_ragged'} rows {rows} {precision}", call, wsb, {"out": Out(B, 768)},
         {"out": want}, 5e-5 if precision == "fp32" else 5e-4)


# ---------------------------------------------------------------- T2M evaluator encoders
def test_t2m_encoders():
    """B = 5, F = 75 (odd; the strided view ld = Cin + 4), m_lens [9, 18, 4, 18, 1], L = 12.  Tolerances: test_gpu_evaluators.py::
    test_gru_lengths_in_any_order_and_odd_frame_counts (movement 2e-5, motion 5e-5) and ::test_encoders_match_reference_golden (text 5e-5)."""
    from ladiff_amd import MotionEncoderBiGRUCo, MovementConvEncoder, TextEncoderBiGRUCo
    mv, mo, tx = syn.t2m_weights(263)
    move = MovementConvEncoder(259, 512, 512); move.load_state_dict(mv, strict=True)
    motion = MotionEncoderBiGRUCo(512, 1024, 512); motion.load_state_dict(mo, strict=True)
    text = TextEncoderBiGRUCo(300, 15, 512, 512); text.load_state_dict(tx, strict=True)
    move, motion, text = move.to(DEV), motion.to(DEV), text.to(DEV)
    gen = torch.Generator().manual_seed(3)
    B, Fr, Lw = 5, 75, 12
    feats = torch.randn(B, Fr, 263, generator=gen)
    m_lens, cap = [9, 18, 4, 18, 1], [12, 3, 7, 1, 9]
    word = torch.randn(B, Lw, 300, generator=gen)
    pos = F.one_hot(torch.randint(0, 15, (B, Lw), generator=gen), 15).float()
    with torch.no_grad():
        mov_o = orc.t2m_movement_encoder(mv, feats)
        mot_o = orc.t2m_motion_encoder(mo, mov_o, torch.tensor(m_lens))
        txt_o = orc.t2m_text_encoder(tx, word, pos, torch.tensor(cap))
    Tm = mov_o.shape[1]
    fd, md, wd, pd, mld, cpd = dev(feats), dev(mov_o.float()), dev(word), dev(pos), ints(m_lens), ints(cap)
    hold("ladiff_t2m_movement_encode",
         lambda ws, nb, o: L().ladiff_t2m_movement_encode(move._table().array, fd.data_ptr(), 263, B, Fr, 259, o["out"], ws, nb, st()),
         L().ladiff_t2m_movement_workspace_bytes(B, Fr, 259), {"out": Out(B * Tm, 512)}, {"out": mov_o}, 2e-5)
    hold("ladiff_t2m_motion_encode",
         lambda ws, nb, o: L().ladiff_t2m_motion_encode(motion._table().array, _lib.ptr(md), mld.data_ptr(), B, Tm, o["out"], ws, nb, st()),
         L().ladiff_t2m_motion_workspace_bytes(B, Tm), {"out": Out(B, 512)}, {"out": mot_o}, 5e-5)
    hold("ladiff_t2m_text_encode",
         lambda ws, nb, o: L().ladiff_t2m_text_encode(text._table().array, _lib.ptr(wd), _lib.ptr(pd), cpd.data_ptr(), B, Lw, o["out"], ws, nb, st()),
         L().ladiff_t2m_text_workspace_bytes(B, Lw), {"out": Out(B, 512)}, {"out": txt_o}, 5e-5)
