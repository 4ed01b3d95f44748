"""WHEN the library captures its hipGraphs (csrc/graph_key.h, csrc/graph_cache.h): an unchanged call replays what it has, a changed one
captures again.  The other GPU tests check the bits of a replay; these count instantiations (`ladiff_debug_graph_instantiations`)
around calls with fixed tensors - a slip in the capture key would otherwise replay a graph with a stale baked-in argument, or capture
on every call, without any result changing.  LADIFF copies its inputs into buffers of the plan (one plan and one sampler per batch
shape), so the pointers a call passes are the same every time."""
import pytest
import torch

from ladiff_amd import LADIFF, DDIMScheduler, LADiffDenoiser, LADiffVae, _lib, synthetic as syn
from test_abi import ABL, DEN_KW, VAE_KW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False)
SHAPES = {2: [196, 60], 3: [196, 60, 120]}              # the shape under test, and the "other" one (its own plan and sampler)


@pytest.fixture(scope="module")
def nets():
    den = LADiffDenoiser(ABL, **DEN_KW); den.load_state_dict(syn.denoiser_weights(), strict=True)
    vae = LADiffVae(ABL, **VAE_KW); vae.load_state_dict(syn.vae_weights(263), strict=True)
    return den.to(DEV).eval(), vae.to(DEV).eval()


def make_pipe(nets, loop):
    den, vae = nets
    return LADIFF(denoiser=den, vae=vae, scheduler=DDIMScheduler(set_alpha_to_one=False, steps_offset=1, **SCHED_KW), guidance_scale=7.5,
                  num_inference_timesteps=2, eta=0.0, max_it=5, precision="f16x3", loop=loop)


def counted(fn):
    """(result, graph instantiations of the library during fn)"""
    L = _lib.lib()
    before = L.ladiff_debug_graph_instantiations()
    out = fn()
    torch.cuda.synchronize()
    return out, L.ladiff_debug_graph_instantiations() - before


@pytest.mark.parametrize("loop,per_capture", [("launches", 2), ("pipeline", 1)])
def test_sampler_captures_when_the_key_or_the_epoch_changes_and_only_then(nets, loop, per_capture):
    """launch-per-stage: a prologue graph and a step graph per capture; pipeline loop: the prologue graph only (the steps are one kernel)."""
    L = _lib.lib()
    pipe = make_pipe(nets, loop)
    data = {B: (syn.text_embeddings(B, seed=B).to(DEV), syn.init_noise(lens, seed=B + 1).to(DEV)) for B, lens in SHAPES.items()}

    def call(B):
        def fn():
            z = pipe._diffusion_reverse(data[B][0], SHAPES[B], init_noise=data[B][1])
            assert pipe.loop_status() == (0, 0)
            assert pipe.last_loop()[0] == (loop != "launches")
            return z
        return counted(fn)

    first, n = call(2)
    print(f"{loop}: first call of a shape: +{n}")
    assert n == per_capture
    z, n = call(2)
    print(f"{loop}: same call again: +{n}")
    assert n == 0 and torch.equal(z, first)
    _, n_other = call(3)
    z, n = call(2)
    print(f"{loop}: the other shape: +{n_other}, then the first shape again: +{n}")
    assert n_other == per_capture                              # a first call of ITS shape
    assert n == per_capture and torch.equal(z, first)          # the epoch rule: another sampler has instantiated since
    try:
        assert L.ladiff_debug_set_graph_epoch_rule(0) == 0
        _, n_other = call(3)
        z, n = call(2)
        print(f"{loop}: epoch rule off: the other shape: +{n_other}, the first shape again: +{n}")
        assert n_other == 0 and n == 0 and torch.equal(z, first)
    finally:
        L.ladiff_debug_set_graph_epoch_rule(1)
    pipe.guidance_scale = 5.0                                  # a scalar baked into the graphs' (the stage table's) arguments
    z5, n = call(2)
    print(f"{loop}: another guidance_scale: +{n}")
    assert n == per_capture and not torch.equal(z5, first)
    z, n = call(2)
    assert n == 0 and torch.equal(z, z5)
    pipe.guidance_scale = 7.5
    z, n = call(2)
    assert n == per_capture and torch.equal(z, first)


def test_decode_graph_captures_when_the_key_or_the_epoch_changes_and_only_then(nets):
    L = _lib.lib()
    _, vae = nets
    lens = [60, 60]                                            # B = 2, F = 60
    z = torch.randn(5, 2, 256, generator=torch.Generator().manual_seed(7)).to(DEV)
    z[2:] = 0                                                  # 60 frames: two latents
    old_rows, old_precision = vae.graph_rows, vae.precision
    vae.graph_rows, vae.precision = 4096, "f16x3"
    try:
        first, n = counted(lambda: vae.decode(z, lens))
        print(f"decode: first call: +{n}")
        assert n == 1
        again, n = counted(lambda: vae.decode(z, lens))
        print(f"decode: repeat: +{n}")
        assert n == 0 and torch.equal(again, first)
        pipe = make_pipe(nets, "pipeline")
        _, n = counted(lambda: pipe._diffusion_reverse(syn.text_embeddings(2, seed=2).to(DEV), SHAPES[2],
                                                       init_noise=syn.init_noise(SHAPES[2], seed=3).to(DEV)))
        assert n >= 1                                          # a sampler has instantiated in between
        again, n = counted(lambda: vae.decode(z, lens))
        print(f"decode: after a sampler's instantiation: +{n}")
        assert n == 1 and torch.equal(again, first)
        try:
            assert L.ladiff_debug_set_decoder_fusion(1 + 8) == 0   # final_layer on the fp32 kernel: a switch that is part of the key
            _, n = counted(lambda: vae.decode(z, lens))
            print(f"decode: after a fusion switch flipped: +{n}")
            assert n == 1
        finally:
            L.ladiff_debug_set_decoder_fusion(1)
        again, n = counted(lambda: vae.decode(z, lens))
        assert n == 1 and torch.equal(again, first)             # the switch is back: the key changed again
        try:
            assert L.ladiff_debug_set_decoder_fusion(1 + 64) == 0  # out_proj + cross-attention as two launches: part of the key as well
            crossed, n = counted(lambda: vae.decode(z, lens))
            print(f"decode: after the out_cross switch flipped: +{n}")
            assert n == 1
            vae.graph_rows = 0                                  # the same decode launched directly, under the same switch
            direct, n = counted(lambda: vae.decode(z, lens))
            assert n == 0 and torch.equal(crossed, direct)
        finally:
            vae.graph_rows = 4096
            L.ladiff_debug_set_decoder_fusion(1)
        again, n = counted(lambda: vae.decode(z, lens))
        assert n == 1 and torch.equal(again, first)             # switched back: captured once more, the first result again
    finally:
        vae.graph_rows, vae.precision = old_rows, old_precision
