"""The LA-VAE decode with its nine cross-attention maps as a second result.  TEST INFRASTRUCTURE ONLY (a plain helper module).

`oracle.skip_decoder` / `oracle.vae_decode` restated on the oracle's own helpers, with ONE difference: the cross-attention of a block runs
through `torch.nn.functional.multi_head_attention_forward(..., need_weights=True, average_attn_weights=True)` - the function the
reference's `nn.MultiheadAttention` layer calls (cross_attention.py:373-376) - and its head-averaged weights [B, F, T] are kept
(:378-406 draws exactly that tensor).  tests/test_att_maps.py holds the restatement's `feats` to `oracle.vae_decode` at 1e-12 in fp64, so
the maps belong to the pinned activations.

Frames past a sample's length are zeroed in the maps, as the product writes them (the reference computes weights there too: the one
documented deviation).  Latents past a sample's count are masked keys: their weight is exactly 0.

`CASES` are the shapes of tests/test_gpu_att_maps.py; `case_inputs` / `reference` build a case's latents and its fp64 / fp32 results once
per process."""
import torch
import torch.nn.functional as F

from ladiff_amd import synthetic as syn
from oracle import ladiff_oracle as orc
from trained_like import oracle_pair, trained_like

NAMES = tuple([f"input_block_{i}" for i in range(4)] + ["middle_block"] + [f"output_block_{i}" for i in range(4)])


def cross_attention(tgt, memory, p, mem_pad, num_heads=orc.NUM_HEADS, average=True):
    """(out_proj(attention) [B,F,D], head-averaged weights [B,F,T]) of nn.MultiheadAttention(query=tgt, key=memory, value=memory);
    average=False: the weights per head, [B,H,F,T]."""
    out, w = F.multi_head_attention_forward(
        tgt.transpose(0, 1), memory.transpose(0, 1), memory.transpose(0, 1), tgt.shape[-1], num_heads,
        p["in_proj_weight"], p["in_proj_bias"], None, None, False, 0.0, p["out_proj.weight"], p["out_proj.bias"],
        training=False, key_padding_mask=mem_pad, need_weights=True, attn_mask=None, average_attn_weights=average)
    return out.transpose(0, 1), w


def decoder_layer(tgt, memory, p, tgt_pad, mem_pad, average=True):
    """oracle.decoder_layer, returning the cross-attention weights as well."""
    a = orc.mha(tgt, tgt, tgt, orc.sub(p, "self_attn"), tgt_pad)
    tgt = orc.layer_norm(tgt + a, p["norm1.weight"], p["norm1.bias"])
    c, w = cross_attention(tgt, memory, orc.sub(p, "multihead_attn"), mem_pad, average=average)
    tgt = orc.layer_norm(tgt + c, p["norm2.weight"], p["norm2.bias"])
    f = orc.linear(F.gelu(orc.linear(tgt, p["linear1.weight"], p["linear1.bias"])), p["linear2.weight"], p["linear2.bias"])
    return orc.layer_norm(tgt + f, p["norm3.weight"], p["norm3.bias"]), w


def skip_decoder(x, memory, p, tgt_pad, mem_pad, num_layers=9, average=True):
    """oracle.skip_decoder -> (x, [the nine maps in execution order])."""
    nb = (num_layers - 1) // 2
    xs, maps = [], []
    for i in range(nb):
        x, w = decoder_layer(x, memory, orc.sub(p, f"input_blocks.{i}"), tgt_pad, mem_pad, average)
        xs.append(x)
        maps.append(w)
    x, w = decoder_layer(x, memory, orc.sub(p, "middle_block"), tgt_pad, mem_pad, average)
    maps.append(w)
    for i in range(nb):
        x = torch.cat([x, xs.pop()], dim=-1)
        x = orc.linear(x, p[f"linear_blocks.{i}.weight"], p[f"linear_blocks.{i}.bias"])
        x, w = decoder_layer(x, memory, orc.sub(p, f"output_blocks.{i}"), tgt_pad, mem_pad, average)
        maps.append(w)
    return orc.layer_norm(x, p["norm.weight"], p["norm.bias"]), maps


def vae_decode(sd, z, lengths, frame_per_latent=48, num_layers=9, latent_counts=None, average=True):
    """oracle.vae_decode -> (feats [B,F,C], maps [9,B,F,T]); frames >= lengths[b] are zero in both.  average=False: the weights of the
    four heads, maps [9,B,H,F,T] (what the head average is taken over)."""
    dtype = z.dtype
    mask = orc.lengths_to_mask(lengths)
    counts = orc.max_iter_elements(lengths, frame_per_latent) if latent_counts is None else latent_counts
    B, Fr = mask.shape
    mem = z.permute(1, 0, 2)
    mem_pad = ~orc.count_mask(counts, mem.shape[1])
    q = torch.zeros(B, Fr, z.shape[-1], dtype=dtype) + sd["query_pos_decoder.pe"][:Fr, 0][None]
    out, maps = skip_decoder(q, mem, orc.sub(sd, "decoder"), ~mask, mem_pad, num_layers, average)
    out = orc.linear(out, sd["final_layer.weight"], sd["final_layer.bias"])
    keep = mask[:, :, None].to(dtype)
    return out * keep, torch.stack(maps) * (keep[None] if average else keep[None, :, None])


# ---------------------------------------------------------------- the cases of the GPU test, and their references (computed once)
LENS_A = [1, 17, 48, 49, 196]                                   # counts 1, 1, 1, 2, 5; F = 196 is no multiple of 16; a one-frame sample
LENS_D = [196] * 20 + [150, 60]                                 # 22 prompts, 4,130 ragged rows of 22 x 196 = 4,312
# name: lengths, max_it, frame_per_latent, length_aware, latentwise_gen, test_efficiency
CASES = {
    "a_ragged_small": dict(lens=LENS_A, T=5, fpl=48, length_aware=True),
    "b_padded_small": dict(lens=LENS_A, T=5, fpl=48, length_aware=False),
    "c_padded_4116_rows": dict(lens=[196] * 21, T=5, fpl=48, length_aware=True),
    "d_ragged_4130_rows": dict(lens=LENS_D, T=5, fpl=48, length_aware=True),
    "e_max_it_8": dict(lens=[196, 25, 26, 100, 1, 176], T=8, fpl=25, length_aware=True),
    "e_max_it_1": dict(lens=[60, 1, 33], T=1, fpl=224, length_aware=True),
    "f_latentwise_fw": dict(lens=[100] * 5, T=5, fpl=48, length_aware=True, latentwise_gen="fw"),
    "g_test_efficiency": dict(lens=[60, 196, 5], T=5, fpl=48, length_aware=True, test_efficiency=True),
}
SEED = 1
_SD, _REF = {}, {}


def weights(kind, T):
    """`synthetic` (constructor-like) or `trained_like` (peaked softmax, spread LayerNorm) LA-VAE weights for max_it = T, 263 features."""
    key = (kind, T)
    if key not in _SD:
        sd = syn.vae_weights(263, max_it=T)
        _SD[key] = trained_like(sd, SEED) if kind == "trained_like" else sd
    return _SD[key]


def case_inputs(name):
    """(z [T,B,256] fp32, lengths, latent counts the decode masks with) of a case."""
    c = CASES[name]
    lens, T, fpl = c["lens"], c["T"], c["fpl"]
    z = torch.randn(T, len(lens), 256, generator=torch.Generator().manual_seed(11 + len(lens) + T))
    if c.get("latentwise_gen") == "fw":                         # ladiff.py:274-283: sample idx keeps its first idx + 1 latents
        counts = list(range(1, T + 1))
        z = z[:, :1].repeat(1, T, 1)
    elif c.get("test_efficiency"):
        counts = [T] * len(lens)                                # no mask: every latent is a key, none is zeroed
    else:
        counts = orc.max_iter_elements(lens, fpl)
    if not c.get("test_efficiency"):
        for i, n in enumerate(counts):
            z[n:, i] = 0
    return z, lens, counts


def reference(name, kind):
    """((feats, maps) in fp64, [e32 of feats, e32 of maps]) of a case on `kind` weights: trained_like.oracle_pair on the restatement."""
    key = (name, kind)
    if key not in _REF:
        z, lens, counts = case_inputs(name)
        c = CASES[name]
        _REF[key] = oracle_pair(lambda dt, sd: vae_decode(sd, z.to(dt), lens, frame_per_latent=c["fpl"], latent_counts=counts),
                                weights(kind, c["T"]))
    return _REF[key]
