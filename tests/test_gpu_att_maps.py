"""Decoder cross-attention maps on the GPU (ladiff_vae_decode_att_maps, LADiffVae.decode(return_att_maps / plot_att_map)) against the fp64
restatement that carries them (tests/att_maps_ref.py), in fp32 and f16x3 mode, on synthetic and trained-like weights.

Gate: trained_like.bound(e32, want, precision, split format) with e32 = max |fp32 restatement - fp64 restatement| of the MAPS of the very
case (trained_like.oracle_pair) - the rule of every trained-like test, applied to the maps as a result of their own.  Every case prints
error, e32 and error / bound (`pytest -s`).  Properties on every case: masked latents and padded frames are bitwise 0.0, values lie in
[0, 1], |row sum - 1| <= 4e-6 (the mean of four fp32 softmaxes over at most 8 terms: about T + 2 roundings of 2^-24, headroom 8).

Bits: the maps decode makes the ordinary decode's launches plus nine, so its frames are bit-identical to the ordinary decode's - except
on the f16x3 large-row route, where the ordinary decode runs the fused out_proj + cross-attention kernel and the maps decode its two
launches: there they are bit-identical to the ordinary decode with that kernel switched off, and within the decode's bound."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import att_maps_ref as ref
from ladiff_amd import LADIFF, DDIMScheduler, LADiffDenoiser, LADiffVae, _lib, synthetic as syn
from ladiff_amd.schema import ABL, DEN_KW, VAE_KW
from memory_contract import FILLS, Out, assert_contract, assert_refused, run_fills, run_in_guards
from trained_like import bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = ["fp32", "f16x3"]
KINDS = ["synthetic", "trained_like"]
ROW_SUM_TOL = 4e-6
LARGE_ROWS = 4096                         # from here the f16x3 decode runs its large-row kernels (the fused out_proj + cross among them)
NO_OUT_CROSS = 1 + 64                     # ladiff_debug_set_decoder_fusion: out_proj GEMM + cross-attention row kernel as two launches
SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False)
_VAE = {}


def lib():
    return _lib.lib()


def make_vae(kind, T, fpl):
    key = (kind, T, fpl)
    if key not in _VAE:
        abl = SimpleNamespace(**{**vars(ABL), "MAX_IT": T, "FRAME_PER_LATENT": fpl})
        m = LADiffVae(abl, **VAE_KW)
        m.load_state_dict(ref.weights(kind, T), strict=True)
        _VAE[key] = m.to(DEV).eval()
    return _VAE[key]


def decode(name, kind, precision, fusion=None, **kw):
    """vae.decode of a case (its route, mask and latentwise mode set on the module for the call) -> the call's result."""
    c = ref.CASES[name]
    vae = make_vae(kind, c["T"], c["fpl"])
    z, lens, _ = ref.case_inputs(name)
    vae.precision, vae.length_aware, vae.graph_rows = precision, c["length_aware"], 0
    vae.test_efficiency = bool(c.get("test_efficiency"))
    try:
        if fusion is not None:
            assert lib().ladiff_debug_set_decoder_fusion(fusion) == 0
        out = vae.decode(z.to(DEV), lens, latentwise_gen=c.get("latentwise_gen"), **kw)
        torch.cuda.synchronize()
    finally:
        lib().ladiff_debug_set_decoder_fusion(1)
        vae.precision, vae.length_aware, vae.test_efficiency = "fp32", True, False
    return out


def rows_of(name):
    c = ref.CASES[name]
    ragged = c["length_aware"] and sum(c["lens"]) < len(c["lens"]) * max(c["lens"])
    return sum(c["lens"]) if ragged else len(c["lens"]) * max(c["lens"])


def check_properties(name, maps):
    """Masked latents and padded frames bitwise 0.0; values in [0, 1]; rows of valid frames sum to 1."""
    _, lens, counts = ref.case_inputs(name)
    bits = maps.contiguous().view(torch.int32)
    assert torch.isfinite(maps).all() and maps.min().item() >= 0.0 and maps.max().item() <= 1.0, name
    worst = 0.0
    for b, (n, cnt) in enumerate(zip(lens, counts)):
        assert int((bits[:, b, :, cnt:] != 0).sum()) == 0, (name, b, "masked latents")
        assert int((bits[:, b, n:] != 0).sum()) == 0, (name, b, "padded frames")
        worst = max(worst, (maps[:, b, :n].double().sum(-1) - 1).abs().max().item())
    assert worst <= ROW_SUM_TOL, (name, worst)
    return worst


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(ref.CASES))
def test_maps_against_the_fp64_restatement(name, kind, precision):
    (want_f, want_m), (e32_f, e32_m) = ref.reference(name, kind)
    feats, maps = decode(name, kind, precision, return_att_maps=True)
    assert maps.dtype == torch.float32 and maps.is_cuda and tuple(maps.shape) == tuple(want_m.shape)
    feats, maps = feats.cpu(), maps.cpu()
    row_sum = check_properties(name, maps)
    fmt = lib().ladiff_split_format()
    err_m, b_m = (maps.double() - want_m).abs().max().item(), bound(e32_m, want_m, precision, fmt)
    err_f, b_f = (feats.double() - want_f).abs().max().item(), bound(e32_f, want_f, precision, fmt)
    print(f"\n[att maps] {name} {kind} {precision} ({rows_of(name)} rows): maps err {err_m:.3e}  e32 {e32_m:.3e}  bound {b_m:.3e}  "
          f"err/bound {err_m / b_m:.3f} | row sum - 1 {row_sum:.2e} | feats err {err_f:.3e}  bound {b_f:.3e}  err/bound {err_f / b_f:.3f}")
    assert err_m <= b_m, (name, kind, precision, err_m, b_m)
    assert err_f <= b_f, (name, kind, precision, err_f, b_f)                    # the decode's own bound
    # bits: the frames of the ordinary decode
    large_split = precision == "f16x3" and rows_of(name) >= LARGE_ROWS
    same = decode(name, kind, precision, fusion=NO_OUT_CROSS if large_split else None).cpu()
    assert torch.equal(feats.view(torch.int32), same.view(torch.int32)), (name, kind, precision)
    if large_split:
        default = decode(name, kind, precision).cpu()
        assert (default.double() - want_f).abs().max().item() <= b_f            # (the fused kernel sums in another order: bits may differ)


def test_large_cases_take_the_large_route():
    assert rows_of("c_padded_4116_rows") == 4116 and rows_of("d_ragged_4130_rows") == 4130
    assert all(rows_of(n) < LARGE_ROWS for n in ref.CASES if n[0] not in "cd")


# ---------------------------------------------------------------- the C entry under the memory contract
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["a_ragged_small", "c_padded_4116_rows"])
def test_memory_contract(name, precision):
    """ladiff_vae_decode_att_maps with feats and att_maps as outputs: refused 4 bytes short, then the three fills at the exact size."""
    kind = "synthetic"
    c = ref.CASES[name]
    (want_f, want_m), (e32_f, e32_m) = ref.reference(name, kind)
    z, lens, counts = ref.case_inputs(name)
    B, Fr, T, C = len(lens), max(lens), c["T"], 263
    vae = make_vae(kind, T, c["fpl"])
    wt = vae._weight_table()
    wsplit = wt.split_array() if precision == "f16x3" else None
    ints = lambda v: torch.tensor(list(v), dtype=torch.int32, device=DEV)
    zd, ld, cd = z.to(DEV).contiguous(), ints(lens), ints(counts)
    ragged = sum(lens) < B * Fr
    off = [0]
    for l in lens:
        off.append(off[-1] + l)
    od = ints(off)

    def call(ws, nb, o):
        return lib().ladiff_vae_decode_att_maps(wt.array, wsplit, _lib.ptr(zd), ld.data_ptr(), cd.data_ptr(), od.data_ptr() if ragged else None,
                                                off[-1] if ragged else 0, B, Fr, T, C, o["feats"], o["att_maps"], ws, nb, _lib.stream_ptr())
    outs = {"feats": Out(B * Fr, C), "att_maps": Out(9 * B * Fr, T)}
    wsb = lib().ladiff_decoder_workspace_bytes(B, Fr, T, C)
    fmt = lib().ladiff_split_format()
    tol = {"feats": bound(e32_f, want_f, precision, fmt), "att_maps": bound(e32_m, want_m, precision, fmt)}
    what = f"ladiff_vae_decode_att_maps {name} {precision}"
    assert_refused(run_in_guards(call, wsb - 4, outs, FILLS["nan"]), what + ", workspace 4 bytes short")
    rep = assert_contract(run_fills(call, wsb, outs), {"feats": want_f, "att_maps": want_m}, tol, what)
    print(f"\nmemory contract | {what}: guard words touched {rep['guards']}, gap words touched {rep['gaps']}, "
          f"fills bit-identical: {rep['identical']}, deterministic: {rep['deterministic']}")
    assert rep["identical"] and rep["deterministic"]


def test_argument_errors_return_before_any_launch():
    vae = make_vae("synthetic", 5, 48)
    wt = vae._weight_table()
    fake = 256
    call = lambda **k: lib().ladiff_vae_decode_att_maps(
        wt.array, None, k.get("z", fake), fake, fake, None, 0, k.get("B", 2), k.get("F", 60), k.get("T", 5), 263, fake, k.get("maps", fake), fake,
        k.get("ws", lib().ladiff_decoder_workspace_bytes(2, 60, 5, 263)), None)
    assert call(maps=None) == -1 and call(z=None) == -1 and call(B=-1) == -1                 # LADIFF_ERR_ARG
    assert call(F=0) == -2 and call(F=225) == -2 and call(T=9) == -2 and call(T=0) == -2      # LADIFF_ERR_SHAPE
    assert call(ws=lib().ladiff_decoder_workspace_bytes(2, 60, 5, 263) - 4) == -3             # LADIFF_ERR_WORKSPACE
    assert lib().ladiff_version() == 6


# ---------------------------------------------------------------- the Python surface
@pytest.fixture(scope="module")
def model():
    den = LADiffDenoiser(ABL, **DEN_KW)
    den.load_state_dict(syn.denoiser_weights(), strict=True)
    vae = make_vae("synthetic", 5, 48)
    dm = SimpleNamespace(feats2joints=lambda f: f)            # identity "joints": the decoded features themselves
    enc_out = torch.randn(2, 1, 768, generator=torch.Generator().manual_seed(96))
    m = LADIFF(None, dm, denoiser=den.to(DEV).eval(), vae=vae, text_encoder=lambda texts: enc_out.to(DEV), guidance_scale=7.5,
               num_inference_timesteps=5, scheduler=DDIMScheduler(set_alpha_to_one=False, steps_offset=1, **SCHED_KW))
    return m, enc_out


@pytest.mark.parametrize("graph_rows", [0, 1 << 20])
def test_forward_writes_nine_files(model, tmp_path, graph_rows):
    """forward(batch, plot_att_map=dir) with B = 1: nine [F,T] files holding the maps of the z it decoded; a module that replays its
    small decodes from a graph still makes the maps call."""
    m, enc_out = model
    length = 77
    noise = syn.init_noise([length], seed=95)
    orig = m._diffusion_reverse
    m._diffusion_reverse = lambda emb, lengths: orig(emb, lengths, init_noise=noise.to(DEV))
    m.vae.graph_rows = graph_rows
    try:
        out = m({"text": ["a person walks"], "length": [length]}, plot_att_map=tmp_path / "maps")
        z = orig(enc_out.to(DEV), [length], init_noise=noise.to(DEV))
        feats, maps = m.vae.decode(z, [length], return_att_maps=True)
    finally:
        m._diffusion_reverse = orig
        m.vae.graph_rows = 0
    assert len(out) == 1 and torch.equal(out[0].cpu(), feats[0].cpu())
    for l, name in enumerate(LADiffVae.att_map_names):
        got = np.load(tmp_path / "maps" / (name + ".npy"))
        assert got.shape == (length, 5) and np.array_equal(got, maps[l, 0].cpu().numpy())
    assert np.load(tmp_path / "maps" / "middle_block.npy")[:, 2:].max() == 0          # 77 frames: two latents


def test_forward_heat_maps(model, tmp_path):
    pytest.importorskip("matplotlib")
    m, _ = model
    m({"text": ["a person walks"], "length": [50]}, plot_att_map=str(tmp_path))
    for name in LADiffVae.att_map_names:
        with open(tmp_path / (name + ".png"), "rb") as fh:
            assert fh.read(8) == b"\x89PNG\r\n\x1a\n"


def test_forward_latentwise_fw_with_maps(model, tmp_path):
    """The demo's call: forward(batch, latentwise_gen="fw", plot_att_map=dir) - sample k of the five reads its first k + 1 latents."""
    m, _ = model
    out = m({"text": ["a person walks"], "length": [196]}, latentwise_gen="fw", plot_att_map=tmp_path)
    assert len(out) == 5
    got = np.load(tmp_path / "output_block_3.npy")
    assert got.shape == (5, 196, 5)
    for k in range(5):
        assert got[k, :, k + 1:].max(initial=0.0) == 0 and abs(got[k].sum(-1) - 1).max() <= ROW_SUM_TOL


def test_sample_returns_the_maps_of_its_latents(model):
    m, enc_out = model
    lens = [60, 196]
    text, noise = syn.text_embeddings(2), syn.init_noise(lens)
    z, feats, maps = m.sample(text.to(DEV), lens, init_noise=noise.to(DEV), return_att_maps=True)
    z2, feats2 = m.sample(text.to(DEV), lens, init_noise=noise.to(DEV))
    assert torch.equal(z, z2) and torch.equal(feats, feats2)
    f3, maps3 = m.vae.decode(z, lens, return_att_maps=True)
    assert tuple(maps.shape) == (9, 2, 196, 5) and torch.equal(maps, maps3) and torch.equal(feats, f3)
    assert maps[:, 0, 60:].abs().max().item() == 0 and maps[:, 0, :, 2:].abs().max().item() == 0


def test_cpu_tensors_raise(model):
    m, _ = model
    with pytest.raises(_lib.LadiffHipError):
        m.vae.decode(torch.zeros(5, 1, 256), [60], return_att_maps=True)
