"""The decoder layer from the self-attention output to the layer output as ONE kernel (csrc/dec_post.hip, dec_post_kernel: out_proj +
norm1 + cross-attention + norm2 + the feed-forward block + norm3 on the feed-forward kernel's weight-streaming skeleton, f16x3 mode,
DecRoute::post) against the two launches it replaces (`ladiff_debug_set_decoder_fusion(.. + 128)`) and against the CPU oracle.
Reference: TransformerDecoderLayer.forward_post, operator/cross_attention.py:367-376, :407-412.

Every case is a decode of a few hundred rows with the fused forms forced at every size: switch value 2 + 4.  (2 alone - the feed-forward
fused always - leaves a decode below 4,096 rows on the small-M route, where neither the fused out_proj + cross kernel nor this one ever
runs; + 4 takes the large-M forms at any row count, so that `post = out_cross && fused_mlp && !small` holds.  Check (e) below is what
shows that the new kernel really ran.)

Shapes: the smallest at which the kernel can go wrong - a sample shorter than a 16-row tile, exactly one tile, a sample boundary inside
a 128-row workgroup, a workgroup with idle waves, totals that are no multiple of 16 or 128; padded and ragged rows; 1 .. 8 latent
tokens with frame_per_latent chosen so that `counts` masks 0 .. 7 of them.

For every case: (a) two calls give equal bits; (b) frames past a length are exactly 0; (c) error against the oracle at most
5e-4 x max(1, |ref|max) - the bound the fused cross kernel is held to (test_gpu_decoder_fusion.py); (d) that error at most twice the
error of the two-launch route on the same inputs in the same run + 1e-6 x scale; (e) the two routes agree within the bound of (c) and
are NOT bit-equal.  Every case prints its figures (`pytest -s`).

Measured (one MI355X, profiles/dec_post/04_tests_dec_post.log; error against the oracle, one launch / two launches): synthetic weights
5.3e-6 .. 1.17e-5 / 4.7e-6 .. 1.06e-5 over the 48 shape cases (worst ratio 1.29, bound of (d): 2 + 1e-6 scale), one against two launches
2.6e-6 .. 4.9e-6; 251 features 1.00e-5 / 9.9e-6; trained-like weights 8.1e-5 / 1.18e-4, one against two 4.7e-5; bound of (c): 1.4e-3 .. 2.4e-3."""
import pytest
import torch

from ladiff_amd import LADiffVae, _lib, synthetic as syn
from oracle import ladiff_oracle as orc
from test_abi import ABL, VAE_KW
from trained_like import trained_like

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORCED = 2 + 4                            # fused feed-forward at every size + the large-M forms at every size: DecRoute::post at any row count
POST_OFF = 128                            # out_proj .. norm2 and the feed-forward as two launches: the path before
NO_OUT_CROSS = 64
T_FPL = [(1, 196), (2, 98), (3, 66), (4, 49), (5, 48), (6, 33), (7, 28), (8, 25)]      # as test_gpu_decoder_fusion.py
SHAPES = {"six": [196, 1, 33, 16, 47, 3], "one": [3], "two": [17, 15]}

_VAE, _REF = {}, {}


def weights(kind, nfeats):
    sd = syn.vae_weights(nfeats)
    return trained_like(sd, 1) if kind == "trained_like" else sd


def make_vae(kind="synthetic", nfeats=263):
    if (kind, nfeats) not in _VAE:
        m = LADiffVae(ABL, **{**VAE_KW, "nfeats": nfeats})
        m.load_state_dict(weights(kind, nfeats), strict=True)
        _VAE[(kind, nfeats)] = m.to(DEV).eval()
    return _VAE[(kind, nfeats)]


def inputs(lens, T, fpl):
    z = torch.randn(T, len(lens), 256, generator=torch.Generator().manual_seed(40 + T + len(lens)))
    for i, l in enumerate(lens):
        z[-(-l // fpl):, i] = 0
    return z


def reference(kind, nfeats, lens, T, fpl):
    """The oracle's frames of a case: computed once, shared by its padded and ragged runs, never modified."""
    key = (kind, nfeats, tuple(lens), T, fpl)
    if key not in _REF:
        _REF[key] = orc.vae_decode(weights(kind, nfeats), inputs(lens, T, fpl), lens, frame_per_latent=fpl)
    return _REF[key]


def decodes(vae, z, lens, fpl, ragged, calls):
    """vae.decode once per (switch value, keyword arguments) of `calls`, the module's settings restored afterwards."""
    L = _lib.lib()
    old = (vae.frame_per_latent, vae.length_aware, vae.precision, vae.max_it, vae.graph_rows)
    out = []
    try:
        vae.frame_per_latent, vae.length_aware, vae.precision, vae.graph_rows = fpl, ragged, "f16x3", 0
        with torch.no_grad():
            for fusion, kw in calls:
                assert L.ladiff_debug_set_decoder_fusion(fusion) == 0, fusion
                out.append(vae.decode(z.to(DEV), lens, **kw))
        torch.cuda.synchronize()
    finally:
        L.ladiff_debug_set_decoder_fusion(1)
        vae.frame_per_latent, vae.length_aware, vae.precision, vae.max_it, vae.graph_rows = old
    return out


def run_case(name, kind, nfeats, lens, T, fpl, ragged):
    vae = make_vae(kind, nfeats)
    z = inputs(lens, T, fpl)
    new, again, two = decodes(vae, z, lens, fpl, ragged, [(FORCED, {}), (FORCED, {}), (FORCED + POST_OFF, {})])
    ref = reference(kind, nfeats, lens, T, fpl)
    scale = max(1.0, ref.abs().max().item())
    e_new = (new.cpu() - ref).abs().max().item()
    e_two = (two.cpu() - ref).abs().max().item()
    d = (new - two).abs().max().item()
    print(f"\n[dec_post] {name} {kind} C={nfeats} T={T} {'ragged' if ragged else 'padded'} rows={sum(lens) if ragged else len(lens) * max(lens)}: "
          f"one launch vs oracle {e_new:.3e}, two launches vs oracle {e_two:.3e}, one vs two {d:.3e}, scale {scale:.2f}")
    assert torch.isfinite(new).all() and torch.equal(new.view(torch.int32), again.view(torch.int32))           # (a)
    for i, l in enumerate(lens):                                                                              # (b)
        if l < new.shape[1]:
            assert new[i, l:].abs().max().item() == 0.0, (name, i)
    assert e_new <= 5e-4 * scale, (name, e_new)                                                               # (c)
    assert e_new <= 2 * e_two + 1e-6 * scale, (name, e_new, e_two)                                            # (d)
    assert 0.0 < d <= 5e-4 * scale, (name, d)                                                                 # (e)


@pytest.mark.parametrize("T,fpl", T_FPL)
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_launch_layer_tail(shape, ragged, T, fpl):
    run_case(shape, "synthetic", 263, SHAPES[shape], T, fpl, ragged)


@pytest.mark.parametrize("ragged", [False, True])
def test_one_launch_layer_tail_251_features(ragged):
    run_case("six", "synthetic", 251, SHAPES["six"], 5, 48, ragged)


@pytest.mark.parametrize("ragged", [False, True])
def test_one_launch_layer_tail_on_trained_like_weights(ragged):
    """Peaked softmax, spread LayerNorm gamma / beta / biases (tests/trained_like.py), under the same bounds."""
    run_case("six", "trained_like", 263, SHAPES["six"], 5, 48, ragged)


@pytest.mark.parametrize("ragged", [False, True])
def test_a_maps_call_takes_the_launches_of_before(ragged):
    """With the cross-attention maps requested the fused out_proj + cross kernel is off for the call, and this kernel with it: the frames
    are those of the call with the new switch off, and of the plain decode on the two-launch GEMM + row-kernel route, bit for bit."""
    lens, T, fpl = SHAPES["six"], 5, 48
    vae = make_vae()
    z = inputs(lens, T, fpl)
    (f_on, m_on), (f_off, m_off), plain = decodes(vae, z, lens, fpl, ragged, [
        (FORCED, {"return_att_maps": True}), (FORCED + POST_OFF, {"return_att_maps": True}), (FORCED + NO_OUT_CROSS + POST_OFF, {})])
    assert torch.equal(f_on.view(torch.int32), f_off.view(torch.int32)) and torch.equal(m_on.view(torch.int32), m_off.view(torch.int32))
    assert torch.equal(f_on.view(torch.int32), plain.view(torch.int32))


def test_switch_values():
    L = _lib.lib()
    try:
        assert L.ladiff_debug_set_decoder_fusion(1 + 128) == 0 and L.ladiff_debug_set_decoder_fusion(128 + 64 + 32 + 8 + 4 + 2) == 0
        assert L.ladiff_debug_set_decoder_fusion(255) != 0 and L.ladiff_debug_set_decoder_fusion(256) != 0
        assert L.ladiff_debug_set_decoder_fusion(3 + 128) != 0 and L.ladiff_debug_set_decoder_fusion(128 + 16 + 32) != 0
    finally:
        L.ladiff_debug_set_decoder_fusion(1)
