"""Model-level GPU parity on trained-like weights (tests/trained_like.py: peaked softmax, spread LayerNorm gamma / beta / biases).

The kernels the product runs by default (in_proj inside the attention kernel, out_proj + cross-attention + two LayerNorms, the fused
feed-forward block, the denoiser's fused attention and hoisted tables, the pipeline kernel's attention and LayerNorm stages, the encoder,
the CLIP tower, the literal linear cross-attention) have no C entry of their own: they are reached through the modules only.  Here the
modules carry weights whose logits reach tens and whose LayerNorms differ per channel and per norm, and every result is compared with
the oracle (oracle/ladiff_oracle.py) in fp64, computed on the CPU at test time.

Bounds (trained_like.bound): e32 = max |oracle fp32 - oracle fp64| of the very case is the unit; fp32 mode 8 e32 + 1e-6 scale, split
mode 8 x (fp16 pairs) or 256 x (bf16 pairs) the e32 term.  Every case prints err, e32 and err / e32 (`pytest -s`)."""
import time
from types import SimpleNamespace

import pytest
import torch

from ladiff_amd import LADIFF, DDIMScheduler, LADiffDenoiser, LADiffVae, _lib, synthetic as syn
from ladiff_amd.text_encoder import MldTextEncoder
from oracle import ladiff_oracle as orc
from conftest import load_golden
from test_abi import ABL, DEN_KW, VAE_KW
from trained_like import bound, oracle_pair, trained_like

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 1
FRAME_TOL = 1e-3          # the absolute gate of tests/test_gpu_path.py on decoded frames: applies as well where the frames are O(1)
PRECISIONS = ["fp32", "f16x3"]
LENS9 = [196, 60, 120, 1, 77, 196, 48, 150, 33]
LENS12 = [196, 60, 120, 1, 77, 196, 48, 150, 33, 32, 64, 65]          # both sides of the 32-row tile edges
SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False)

_ORACLE = {}
_CPU = {"seconds": 0.0}


def lib():
    return _lib.lib()


def oracle(key, fn, *sds):
    """(fp64 results, e32 per result) of a case, computed once for all its precision / routing parametrisations."""
    if key not in _ORACLE:
        t = time.time()
        _ORACLE[key] = oracle_pair(fn, *sds)
        _CPU["seconds"] += time.time() - t
    return _ORACLE[key]


def check(name, precision, got, want, e32, gate=None):
    got = got.detach().double().cpu()
    assert got.shape == want.shape and torch.isfinite(got).all(), name
    err = (got - want).abs().max().item()
    b = bound(e32, want, precision, lib().ladiff_split_format())
    print(f"\n[trained-like] {name}, {precision}: err {err:.3e}  e32 {e32:.3e}  err/e32 {err / max(e32, 1e-30):7.2f}  bound {b:.3e}  "
          f"max|want| {want.abs().max().item():.2f}  (oracle CPU time so far {_CPU['seconds']:.0f} s)")
    assert err <= b, (name, precision, err, b)
    # the absolute gate of the existing tests, where the outputs are O(1) AND the fp32 bound itself lies inside the gate: where a plain
    # fp32 evaluation of the oracle already misses it (the guided loop on peaked weights amplifies rounding: e32 of the frames reaches
    # 1e-2 at 43 prompts), the gate says nothing about a kernel
    if gate is not None and want.abs().max().item() < 16 and 8 * e32 < gate:
        # the gate is a number for fp16 pairs (2^-21 per operand); in split mode on the bf16-pair build (2^-16) it is 32 x that, the
        # ratio of the two terms of trained_like.bound (measured there: 1.0e-3 ... 1.5e-3 on three decodes, profiles/bf16_suite)
        if precision != "fp32" and lib().ladiff_split_format() == 0:
            gate = 32 * gate
        assert err < gate, (name, precision, err)
    return err


# ---------------------------------------------------------------- weights and modules
_SD = {}


def weights(kind, *args):
    key = (kind,) + args
    if key not in _SD:
        if kind == "vae":
            nfeats, max_it = args
            _SD[key] = trained_like(syn.vae_weights(nfeats, max_it=max_it), SEED)
        elif kind == "den":
            _SD[key] = trained_like(syn.denoiser_weights(), SEED)
        else:
            _SD[key] = trained_like(syn.clip_weights(*args), SEED)
    return _SD[key]


_VAE = {}


def make_vae(nfeats=263, max_it=5, fpl=48):
    key = (nfeats, max_it, fpl)
    if key not in _VAE:
        abl = SimpleNamespace(**{**vars(ABL), "MAX_IT": max_it, "FRAME_PER_LATENT": fpl})
        m = LADiffVae(abl, **{**VAE_KW, "nfeats": nfeats})
        m.load_state_dict(weights("vae", nfeats, max_it), strict=True)
        _VAE[key] = m.to(DEV).eval()
    m = _VAE[key]
    m.precision, m.length_aware, m.graph_rows = "fp32", True, 0
    return m


@pytest.fixture(scope="module")
def denoiser():
    m = LADiffDenoiser(ABL, **DEN_KW)
    m.load_state_dict(weights("den"), strict=True)
    return m.to(DEV).eval()


def test_split_range_check_passes_on_trained_like_weights(denoiser):
    """Every operand the split mode converts is finite and inside the fp16 halves' exact range (what the checkpoint loader checks)."""
    for m, kinds in ((make_vae(), ("decoder", "encoder")), (denoiser, ("denoiser",))):
        for kind in kinds:
            rep = m._weight_table(kind).range_report()
            assert rep and all(r["nonfinite"] == 0 and r["beyond_range"] == 0 and r["max_abs"] < 65504 / 1024 for r in rep.values()), kind


# ---------------------------------------------------------------- LA-VAE decoder
def latents(lens, T=5, fpl=48, seed=4):
    z = torch.randn(T, len(lens), 256, generator=torch.Generator().manual_seed(seed + len(lens)))
    for i, l in enumerate(lens):
        z[-(-l // fpl):, i] = 0
    return z


def decode_case(name, precision, lens, nfeats=263, T=5, fpl=48, length_aware=True, fusion=None, mlp_variant=None, graph_rows=0):
    vae = make_vae(nfeats, T, fpl)
    z = latents(lens, T, fpl)
    (want,), (e32,) = oracle(("decode", nfeats, T, fpl, tuple(lens)),
                             lambda dt, sd: orc.vae_decode(sd, z.to(dt), lens, frame_per_latent=fpl), weights("vae", nfeats, T))
    vae.precision, vae.length_aware, vae.graph_rows = precision, length_aware, graph_rows
    try:
        if fusion is not None:
            assert lib().ladiff_debug_set_decoder_fusion(fusion) == 0, fusion
        if mlp_variant is not None:
            assert lib().ladiff_debug_set_mlp_variant(mlp_variant) == 0, mlp_variant
        got = vae.decode(z.to(DEV), lens)
        torch.cuda.synchronize()
    finally:
        lib().ladiff_debug_set_decoder_fusion(1)
        lib().ladiff_debug_set_mlp_variant(0)
        vae.precision, vae.length_aware, vae.graph_rows = "fp32", True, 0
    for i, l in enumerate(lens):
        if l < got.shape[1]:
            assert got[i, l:].abs().max().item() == 0, (name, i)
    check(f"decode {name}", precision, got, want, e32, gate=FRAME_TOL)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("length_aware", [True, False])
@pytest.mark.parametrize("nfeats,lens", [(263, LENS9), (251, LENS9), (263, LENS12), (251, [224, 200, 31]), (263, [1])])
def test_decoder_small_batches(nfeats, lens, length_aware, precision):
    decode_case(f"C={nfeats} B={len(lens)} F={max(lens)} {'ragged' if length_aware else 'padded'}", precision, lens, nfeats,
                length_aware=length_aware)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("fusion", [0, 1, 2, 1 + 4, 1 + 8, 1 + 16, 1 + 32, 1 + 64])
def test_decoder_every_kernel_routing(fusion, precision):
    """`ladiff_debug_set_decoder_fusion`: feed-forward as three launches / fused from 10,000 rows / fused always, large-M GEMMs at few
    rows, final_layer on the fp32-input kernel, in_proj outside / inside the attention kernel, out_proj + cross-attention unfused."""
    decode_case(f"routing {fusion} ragged", precision, LENS12, fusion=fusion)
    decode_case(f"routing {fusion} padded", precision, LENS9, 251, length_aware=False, fusion=fusion)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,lens,nfeats,length_aware", [
    ("4,905 ragged rows", LENS9 * 5, 263, True), ("8,820 padded rows", LENS9 * 5, 251, False), ("10,791 ragged rows", LENS9 * 11, 263, True),
    ("10,780 padded rows", LENS9 * 6 + [196], 263, False)])
def test_decoder_default_kernels_at_size(name, lens, nfeats, length_aware, precision):
    """Above 4,096 frame rows the defaults are in_proj inside the attention kernel, out_proj + cross-attention + LayerNorms in one kernel
    and final_layer on padded tiles; above 10,000 the fused feed-forward block as well."""
    decode_case(name, precision, lens, nfeats, length_aware=length_aware)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_decoder_fused_mlp_variants(variant):
    decode_case(f"fused MLP variant {variant}", "f16x3", LENS12, fusion=2, mlp_variant=variant)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("T,fpl", [(1, 224), (3, 80), (8, 25)])
def test_decoder_memory_token_counts(T, fpl, precision):
    decode_case(f"T={T} memory tokens ragged", precision, LENS9, T=T, fpl=fpl)
    decode_case(f"T={T} memory tokens, in_proj inside + fused MLP", precision, LENS9, T=T, fpl=fpl, fusion=2 + 32)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_decoder_graphed(precision):
    decode_case("graphed ragged", precision, LENS9, graph_rows=4096)
    decode_case("graphed padded", precision, [60] * 8, graph_rows=4096)


# ---------------------------------------------------------------- denoiser forward
def denoiser_case(denoiser, name, precision, B, T, masked, t, n_text=1):
    gen = torch.Generator().manual_seed(1000 * B + 10 * T + n_text)
    x, txt = torch.randn(B, T, 256, generator=gen), torch.randn(B, n_text, 768, generator=gen)
    counts = torch.randint(1, T + 1, (B,), generator=gen) if masked else None
    (want,), (e32,) = oracle(("den", B, T, masked, t, n_text),
                             lambda dt, sd: orc.denoiser_forward(sd, x.to(dt), t, txt.to(dt), counts), weights("den"))
    denoiser.precision = precision
    try:
        got = denoiser(x.to(DEV), torch.tensor(t), txt.to(DEV), max_iter_elements=None if counts is None else counts.to(DEV))[0]
        torch.cuda.synchronize()
    finally:
        denoiser.precision = "fp32"
    check(f"denoiser {name}", precision, got, want, e32)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("t", [981, 1])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("B,T", [(1, 1), (7, 3), (33, 5), (37, 5), (13, 8)])
def test_denoiser_forward(denoiser, B, T, masked, t, precision):
    denoiser_case(denoiser, f"B={B} T={T} {'masked' if masked else 'no mask'} t={t}", precision, B, T, masked, t)


@pytest.mark.parametrize("n_text", [4, 77])
def test_denoiser_forward_many_text_tokens(denoiser, n_text):
    """csrc/linear_ca.hip: the literal linear cross-attention (two more softmaxes), N extra keys in the self-attention."""
    denoiser_case(denoiser, f"N={n_text} text tokens", "fp32", 6, 5, True, 481, n_text)


# ---------------------------------------------------------------- LA-VAE encoder
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,nfeats", [("vae_encode_humanml", 263), ("vae_encode_kit", 251)])
def test_encoder(name, nfeats, precision):
    g = load_golden(name)
    lens = g["lengths"].tolist()
    want, e32 = oracle(("enc", name), lambda dt, sd: orc.vae_encode(sd, g["features"].to(dt), lens, g["eps"].to(dt)),
                       weights("vae", nfeats, 5))
    v = make_vae(nfeats)
    v.precision = precision
    try:
        latent, dist, counts = v.encode(g["features"].to(DEV), lens, eps=g["eps"].to(DEV))
        torch.cuda.synchronize()
    finally:
        v.precision = "fp32"
    for i, c in enumerate(counts.tolist()):
        if c < latent.shape[0]:
            assert latent[c:, i].abs().max().item() == 0
    for what, got, w, e in zip(("mu", "std", "latent"), (dist.loc, dist.scale, latent), want, e32):
        check(f"encoder {name} {what}", precision, got, w, e)


# ---------------------------------------------------------------- CLIP text tower
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("vocab,layers,prompts", [(512, 2, 6), (49408, 12, 2), (49408, 12, 8)])
def test_clip(vocab, layers, prompts, precision):
    """Ragged entry (rows up to the last EOS, unique prompts) and padded entry (77 positions of every row); 2 prompts ragged = the
    few-rows path of the split mode (<= 256 rows), the padded entries of 6 / 8 prompts = the many-rows path."""
    ids = syn.clip_token_ids(prompts, vocab, empty_first=prompts // 2, seed=5)
    sd = weights("clip", vocab, layers)
    (want,), (e32,) = oracle(("clip", vocab, layers, prompts), lambda dt, s: orc.clip_text_features(s, ids, layers), sd)
    enc = MldTextEncoder(vocab_size=vocab, num_layers=layers, precision=precision)
    enc.text_model.load_state_dict(sd, strict=True)
    enc = enc.to(DEV).eval()
    check(f"CLIP {layers} layers, {prompts} prompts, ragged", precision, enc.encode_ids(ids), want, e32)
    check(f"CLIP {layers} layers, {prompts} prompts, padded", precision, enc.encode_ids(ids, full_length=True, dedup=False), want, e32)


# ---------------------------------------------------------------- sampling loop + decode
def loop_case(denoiser, name, precision, B, loop, tagged=True, guidance=7.5):
    lens = [max(1, min(196, 48 * ((i % 5) + 1) - 5 * (i % 3))) for i in range(B)]
    text = syn.text_embeddings(B, seed=900 + B)
    if guidance <= 1.0:
        text = text[B:].contiguous()
    noise = syn.init_noise(lens, seed=901 + B)
    want, e32 = oracle(("loop", B, guidance), lambda dt, den, vae: orc.sample_motions(
        den, vae, text, lens, noise, 5, "ddim", guidance_scale=guidance, dtype=dt), weights("den"), weights("vae", 263, 5))
    vae = make_vae()
    sch = DDIMScheduler(set_alpha_to_one=False, steps_offset=1, **SCHED_KW)
    kw = {} if loop is None else {"loop": loop}
    pipe = LADIFF(denoiser=denoiser, vae=vae, scheduler=sch, guidance_scale=guidance, num_inference_timesteps=5, eta=0.0,
                  precision=precision, **kw)
    assert lib().ladiff_debug_set_handoff(1 if tagged else 0) == 0
    try:
        z, feats = pipe.sample(text.to(DEV), lens, init_noise=noise.to(DEV))
        pipe.check()
        assert pipe.loop_status() == (0, 0)
        if loop is not None and guidance > 1.0:
            assert pipe.last_loop()[0] == (loop != "launches")
    finally:
        lib().ladiff_debug_set_handoff(1)
        denoiser.precision = vae.precision = "fp32"
    for i, l in enumerate(lens):
        c = -(-l // 48)
        if c < 5:
            assert z[c:, i].abs().max().item() == 0
        if l < feats.shape[1]:
            assert feats[i, l:].abs().max().item() == 0
    check(f"loop {name} B={B} latents", precision, z, want[0], e32[0])
    check(f"loop {name} B={B} frames", precision, feats, want[1], e32[1], gate=FRAME_TOL)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("B", [3, 7, 43])
@pytest.mark.parametrize("loop,tagged", [("launches", True), ("pipeline32", True), ("pipeline16", True), ("pipeline16", False),
                                         ("pipeline", True), (None, True)])
def test_sampling_loop(denoiser, loop, tagged, B, precision):
    loop_case(denoiser, f"{loop or 'default'} {'tagged' if tagged else 'flags'}", precision, B, loop, tagged)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_sampling_loop_without_guidance(denoiser, precision):
    loop_case(denoiser, "default, no guidance", precision, 7, None, guidance=1.0)
