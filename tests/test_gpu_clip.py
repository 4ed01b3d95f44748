"""GPU parity of the CLIP text tower against goldens captured from transformers' CLIPModel
(tests/golden/make_golden_clip.py) and against the CPU oracle; plus the two exact host-side shortcuts."""
import pytest
import torch

from ladiff_amd import synthetic as syn
from ladiff_amd.text_encoder import MldTextEncoder
from oracle import ladiff_oracle as orc
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {"fp32": 5e-5, "f16x3": 5e-4}     # outputs are O(1..4); f16x3 keeps 16 significant bits per operand


def make_encoder(vocab, layers, precision="fp32", **kw):
    m = MldTextEncoder(vocab_size=vocab, num_layers=layers, precision=precision, **kw)
    m.text_model.load_state_dict(syn.clip_weights(vocab, layers), strict=True)
    return m.to(DEV).eval()


def maxdiff(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", ["clip_small", "clip_small_eos", "clip_full"])
def test_text_features_match_transformers_golden(name, precision):
    g = load_golden(name)
    enc = make_encoder(int(g["vocab"]), int(g["layers"]), precision)
    out = enc.encode_ids(g["ids"])
    assert out.shape == (g["ids"].shape[0], 768) and out.device.type == "cuda"
    assert maxdiff(out, g["text_features"]) < TOL[precision]


def test_truncation_and_dedup_are_exact():
    g = load_golden("clip_small")
    enc = make_encoder(int(g["vocab"]), int(g["layers"]))
    ids = g["ids"]
    ids = torch.cat([ids, ids[:2], ids[:1]])                       # duplicates, as the guidance batch has
    a = enc.encode_ids(ids)                                         # L = last EOS + 1, unique rows only
    b = enc.encode_ids(ids, full_length=True, dedup=False)          # all 77 positions of every row
    assert torch.equal(a, enc.encode_ids(ids)) and maxdiff(a, b) < 2e-6       # a second call: the same bits; same arithmetic per row, tile shapes may differ
    assert torch.equal(a[0], a[6]) and torch.equal(a[0], a[8]) and torch.equal(a[1], a[7])


def test_few_rows_path_of_the_split_mode_against_the_many_rows_path_and_the_oracle():
    """csrc/clip.hip: up to 256 rows (a demo.py call: "" + one prompt) the split mode's GEMMs run on the K-resident 64x64 tiles with K / 256
    partial planes + a row pass; above, on the large-M tiles.  The same prompts through both (ragged rows: few; every prompt padded to 77
    positions: many) and against the CPU oracle, full 12-layer geometry."""
    vocab, layers = 49408, 12
    sd = syn.clip_weights(vocab, layers)
    ids = syn.clip_token_ids(2, vocab, empty_first=1, seed=5)                # the guidance batch of ONE prompt
    enc = make_encoder(vocab, layers, "f16x3")
    few = enc.encode_ids(ids)                                                # ~3 + n rows
    many = enc.encode_ids(torch.cat([ids] * 3), full_length=True, dedup=False)[:2]   # 6 x 77 = 462 rows
    ref = orc.clip_text_features(sd, ids, layers)
    assert maxdiff(few, ref) < TOL["f16x3"] and maxdiff(many, ref) < TOL["f16x3"]
    from ladiff_amd import _lib
    # the two tilings sum the K parts in different orders: the difference is the split products' own rounding (fp16 pairs 3e-7 per K = 768
    # product, bf16 pairs - LADIFF_TEST_LIB=ladiff_amd/libladiff_hip_bf16.so - 5e-6)
    assert maxdiff(few, many) < (1e-5 if _lib.split_mode_name() == "f16x3" else 1e-4)


def test_guidance_batch_against_oracle():
    """[""] * B + prompts (ladiff.py:258-262) at a batch the oracle finishes in seconds; 4-layer tower, full vocabulary."""
    vocab, layers, B = 49408, 4, 24
    sd = syn.clip_weights(vocab, layers)
    ids = syn.clip_token_ids(2 * B, vocab, empty_first=B)
    enc = make_encoder(vocab, layers)
    out = enc.encode_ids(ids)
    ref = orc.clip_text_features(sd, ids, layers)
    assert maxdiff(out, ref) < TOL["fp32"]
    enc.precision = "f16x3"
    assert maxdiff(enc.encode_ids(ids), ref) < TOL["f16x3"]


def test_forward_with_a_tokenizer_callable():
    """`forward(texts)` follows mld_clip.py:54-78: tokenizer(padding="max_length") -> ids -> [B, 1, 768]."""
    vocab = 512

    class Tok:                                   # stands in for the CLIP BPE tokenizer (vocabulary files are not offline)
        model_max_length = 77

        def __call__(self, texts, padding, truncation, max_length, return_tensors):
            assert padding == "max_length" and truncation and max_length == 77 and return_tensors == "pt"
            ids = torch.full((len(texts), 77), vocab - 1, dtype=torch.int64)
            ids[:, 0] = vocab - 2
            for i, t in enumerate(texts):
                w = [sum(map(ord, x)) % (vocab - 2) for x in t.split()][:75]
                ids[i, 1:1 + len(w)] = torch.tensor(w, dtype=torch.int64)
            return {"input_ids": ids}

    enc = make_encoder(vocab, 2, tokenizer=Tok())
    texts = ["", "a person walks forward", "a person jumps", ""]
    out = enc(texts)
    assert out.shape == (4, 1, 768)
    ref = orc.clip_text_features(syn.clip_weights(vocab, 2), Tok()(texts, "max_length", True, 77, "pt")["input_ids"], 2)
    assert maxdiff(out[:, 0], ref) < TOL["fp32"]


def test_errors_mirror_the_reference():
    with pytest.raises(ValueError, match="not supported"):
        MldTextEncoder("deps/t5-base")                              # mld_clip.py:47-48
    with pytest.raises(NotImplementedError):
        MldTextEncoder("deps/bert-base-uncased")
    with pytest.raises(NotImplementedError):
        MldTextEncoder(last_hidden_state=True)
    enc = make_encoder(512, 2)
    with pytest.raises(IndexError):
        enc.encode_ids(torch.full((1, 77), 600))
    with pytest.raises(Exception, match="tokenizer"):
        enc(["a person walks"])


def test_prompts_to_frames_against_oracle():
    """Token ids -> CLIP -> 5-step guided DDIM -> LA-VAE frames, everything on the HIP path, against the oracle chain;
    the text encoder comes in through the reference's YAML target (mld_clip.MldTextEncoder)."""
    from ladiff_amd import LADIFF
    from test_abi import ABL, DEN_KW, VAE_KW
    vocab, layers, lens = 512, 2, [60, 196, 120]
    cfg = {"model": {"guidance_scale": 7.5,
                     "text_encoder": {"target": "ladiff.models.architectures.mld_clip.MldTextEncoder",
                                      "params": {"finetune": False, "last_hidden_state": False, "latent_dim": [1, 256],
                                                 "vocab_size": vocab, "num_layers": layers}},
                     "denoiser": {"target": "ladiff.models.architectures.ladiff_denoiser.LADiffDenoiser",
                                  "params": {**DEN_KW, "ablation": ABL}},
                     "motion_vae": {"target": "ladiff.models.architectures.ladiff_vae.LADiffVae",
                                    "params": {**VAE_KW, "ablation": ABL}},
                     "scheduler": {"target": "diffusers.DDIMScheduler", "num_inference_timesteps": 5, "eta": 0.0,
                                   "params": dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                                                  beta_schedule="scaled_linear", clip_sample=False,
                                                  set_alpha_to_one=False, steps_offset=1)}},
           "TRAIN": {"ABLATION": {"MAX_IT": 5, "FRAME_PER_LATENT": 48, "TEST_EFFICIENCY": False}}}
    model = LADIFF(cfg, None)
    assert isinstance(model.text_encoder, MldTextEncoder)
    den_sd, vae_sd, clip_sd = syn.denoiser_weights(), syn.vae_weights(263), syn.clip_weights(vocab, layers)
    model.denoiser.load_state_dict(den_sd)
    model.vae.load_state_dict(vae_sd)
    model.text_encoder.text_model.load_state_dict(clip_sd)
    model.to(DEV).eval()
    ids = syn.clip_token_ids(2 * len(lens), vocab, empty_first=len(lens))
    noise = syn.init_noise(lens, seed=41)
    text = model.text_encoder.encode_ids(ids).unsqueeze(1)
    z, feats = model.sample(text, lens, init_noise=noise.to(DEV))
    text_o = orc.clip_text_features(clip_sd, ids, layers).unsqueeze(1)
    z_o, feats_o = orc.sample_motions(den_sd, vae_sd, text_o, lens, noise, 5, "ddim")
    assert maxdiff(text, text_o) < TOL["fp32"]
    assert maxdiff(feats, feats_o) < 1e-3


# the whole chain at the FULL geometry: what `bench.py --config e2e` times
E2E_TOL = 1e-3          # the north-star gate, for the whole chain in BOTH modes (rounds 4 - 5 held the bf16-pair chain to a looser 3e-3)


def test_full_geometry_chain_against_oracle_both_modes():
    """Token ids -> 12-layer CLIP ViT-L/14 text tower (49,408 tokens, random init) -> 50-step guided DDIM -> LA-VAE frames for 16 prompts of
    mixed lengths, both arithmetic modes, against the CPU oracle chain.  The north-star gate (1e-3) is defined on IDENTICAL text embeddings;
    here the embeddings come from the tower in the same arithmetic mode, and the 50-step loop amplifies their rounding (random-init
    weights: |latent| ~ 280): both chains are held to the gate (with bf16 pairs - rounds 4 - 5 - the split chain measured 1.07e-3 on the worst prompt of
    the benchmark batch and had a looser stated 3e-3; with fp16 pairs 2.7e-4).  The loop + decode on the ORACLE's embeddings is held to it as well."""
    from ladiff_amd import LADIFF, DDIMScheduler, LADiffDenoiser, LADiffVae
    from test_abi import ABL, DEN_KW, VAE_KW
    B = 16
    lens = ([196, 60, 120, 196, 100, 196, 48, 150] * 2)[:B]
    den_sd, vae_sd, clip_sd = syn.denoiser_weights(), syn.vae_weights(263), syn.clip_weights()
    ids = syn.clip_token_ids(2 * B, empty_first=B, seed=97)
    noise = syn.init_noise(lens, seed=98)
    with torch.no_grad():
        text_o = orc.clip_text_features(clip_sd, ids, 12).unsqueeze(1)
        z_o, f_o = orc.sample_motions(den_sd, vae_sd, text_o, lens, noise, 50, "ddim")
    den = LADiffDenoiser(ABL, **DEN_KW); den.load_state_dict(den_sd)
    vae = LADiffVae(ABL, **VAE_KW); vae.load_state_dict(vae_sd)
    sch = DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                        set_alpha_to_one=False, steps_offset=1)
    pipe = LADIFF(denoiser=den.to(DEV), vae=vae.to(DEV), scheduler=sch, guidance_scale=7.5, num_inference_timesteps=50)
    enc = MldTextEncoder(precision="fp32")
    enc.text_model.load_state_dict(clip_sd, strict=True)
    enc = enc.to(DEV).eval()
    for precision in ("fp32", "f16x3"):
        pipe.precision = enc.precision = precision
        text = enc.encode_ids(ids.to(DEV)).unsqueeze(1)
        _, feats = pipe.sample(text, lens, init_noise=noise.to(DEV))
        per_prompt = [maxdiff(feats[i, :l], f_o[i, :l]) for i, l in enumerate(lens)]
        worst = max(range(B), key=lambda i: per_prompt[i])
        emb = maxdiff(text, text_o)
        _, feats_same = pipe.sample(text_o.to(DEV), lens, init_noise=noise.to(DEV))        # the gate's own condition: identical embeddings
        same = maxdiff(feats_same, f_o)
        print(f"full-geometry chain, {precision}: embeddings {emb:.2e}, frames worst prompt {worst}: {per_prompt[worst]:.2e}; "
              f"loop + decode on the oracle's embeddings: {same:.2e}")
        assert per_prompt[worst] < E2E_TOL, (precision, per_prompt)
        assert same < 1e-3, (precision, same)
