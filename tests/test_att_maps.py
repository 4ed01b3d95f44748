"""Decoder cross-attention maps, the CPU side: the fp64 restatement that carries the maps (tests/att_maps_ref.py) is held to the pinned
oracle, the properties of the maps are checked on the reference alone, and the Python surface that needs no GPU (the error a CPU tensor
gets, the files `plot_att_map` writes) is checked on the module."""
import os
import warnings

import numpy as np
import pytest
import torch

import att_maps_ref as ref
from ladiff_amd import LADiffVae, _lib, synthetic as syn
from ladiff_amd.schema import ABL, VAE_KW
from oracle import ladiff_oracle as orc

KINDS = ["synthetic", "trained_like"]


def fp64(name, kind):
    (feats, maps), _ = ref.reference(name, kind)
    return feats, maps


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(ref.CASES))
def test_restatement_is_the_pinned_decode(name, kind):
    """feats of the restatement == oracle.vae_decode within 1e-12 in fp64: the maps belong to the activations the goldens pin."""
    feats, maps = fp64(name, kind)
    z, lens, counts = ref.case_inputs(name)
    c = ref.CASES[name]
    sd = {k: v.double() for k, v in ref.weights(kind, c["T"]).items()}
    with torch.no_grad():
        want = orc.vae_decode(sd, z.double(), lens, frame_per_latent=c["fpl"], latent_counts=counts)
    err = (feats - want).abs().max().item()
    print(f"\n[att maps] {name} {kind}: restatement feats - oracle feats {err:.3e}")
    assert feats.dtype == torch.float64 and err <= 1e-12
    assert maps.shape == (9, len(lens), max(lens), c["T"]) and maps.dtype == torch.float64


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(ref.CASES))
def test_reference_maps_are_distributions_over_the_unmasked_latents(name, kind):
    _, maps = fp64(name, kind)
    _, lens, counts = ref.case_inputs(name)
    for b, (n, cnt) in enumerate(zip(lens, counts)):
        assert (maps[:, b, :n].sum(-1) - 1).abs().max().item() <= 1e-12
        assert maps[:, b, :n].min().item() >= 0
        assert (maps[:, b, :, cnt:] == 0).all() and (maps[:, b, n:] == 0).all()


def _measured_case():
    """The decode tests/trained_like.py measured its figures on (tests/test_trained_like.py: 8 motions, latents of seed 4, ceil(len / 48)
    of them per motion)."""
    lens = [196, 60, 120, 1, 77, 48, 150, 33]
    z = torch.randn(5, len(lens), 256, generator=torch.Generator().manual_seed(4))
    counts = orc.max_iter_elements(lens)
    for i, n in enumerate(counts):
        z[n:, i] = 0
    return z, lens, counts, 48, 5


def _case(name):
    if name == "measured_8_motions":
        return _measured_case()
    z, lens, counts = ref.case_inputs(name)
    return z, lens, counts, ref.CASES[name]["fpl"], ref.CASES[name]["T"]


@pytest.mark.parametrize("name,gated", [("measured_8_motions", True), ("a_ragged_small", True), ("d_ragged_4130_rows", False),
                                        ("g_test_efficiency", False)])
def test_trained_like_maps_are_peaked(name, gated):
    """trained_like(sd, 1): the mean largest probability of every layer's softmax - one per head and frame - is at least 0.9 on the decode
    tests/trained_like.py measured as 0.96 .. 0.97 (8 motions with 1 .. 5 unmasked latents, padded frames counted; over the valid frames
    alone it is 0.93 .. 0.96 here) and on case (a).  The figure depends on how many latents compete: where nearly every row has all five
    as keys (d: 0.90 .. 0.94, g, unmasked: 0.86 .. 0.96) it is printed and held to 0.8 - these cases are not the one the 0.9 was stated for.
    The four heads peak on DIFFERENT latents: the largest value of their average, the map, is 0.4 .. 0.7 (printed), and the mean over the
    heads of the per-head weights is the map."""
    z, lens, counts, fpl, T = _case(name)
    sd = {k: v.double() for k, v in ref.weights("trained_like", T).items()}
    with torch.no_grad():
        _, maps = ref.vae_decode(sd, z.double(), lens, frame_per_latent=fpl, latent_counts=counts)
        _, heads = ref.vae_decode(sd, z.double(), lens, frame_per_latent=fpl, latent_counts=counts, average=False)
    assert heads.shape == (9, len(lens), 4) + tuple(maps.shape[2:]) and (heads.mean(2) - maps).abs().max().item() <= 1e-15
    valid = orc.lengths_to_mask(lens)
    top = [heads[l].amax(-1).transpose(0, 1)[:, valid].mean().item() for l in range(9)]
    avg = [maps[l].amax(-1)[valid].mean().item() for l in range(9)]
    print(f"\n[att maps] {name}: mean largest probability per layer {min(top):.3f} .. {max(top):.3f}; of the head average "
          f"{min(avg):.3f} .. {max(avg):.3f}")
    assert min(top) >= (0.9 if gated else 0.8)


def test_some_frames_read_two_latents():
    """At least one case has frames where two latents each hold more than 0.1: the maps are not one-hot rows only."""
    found = {}
    for name in ("a_ragged_small", "g_test_efficiency", "e_max_it_8"):
        for kind in KINDS:
            _, maps = fp64(name, kind)
            found[(name, kind)] = int(((maps > 0.1).sum(-1) >= 2).sum())
    print(f"\n[att maps] frames (over the nine layers) with two latents above 0.1: {found}")
    assert any(found.values())


# ---------------------------------------------------------------- the module, without a GPU
@pytest.fixture(scope="module")
def vae():
    m = LADiffVae(ABL, **VAE_KW)
    m.load_state_dict(syn.vae_weights(263), strict=True)
    return m.eval()


def test_names():
    assert LADiffVae.att_map_names == ref.NAMES and len(LADiffVae.att_map_names) == 9


@pytest.mark.parametrize("kw", [dict(plot_att_map="unused_dir"), dict(return_att_maps=True)])
def test_cpu_tensors_are_refused_like_everywhere(vae, kw, tmp_path):
    """No CPU fallback: a maps decode of CPU tensors raises LadiffHipError (it raised NotImplementedError before the maps were built),
    and writes nothing."""
    from ladiff_amd import build
    build.build()
    if "plot_att_map" in kw:
        kw = dict(plot_att_map=tmp_path / "maps")
    with pytest.raises(_lib.LadiffHipError):
        vae.decode(torch.zeros(5, 2, 256), [60, 30], **kw)
    assert not (tmp_path / "maps").exists()


@pytest.mark.parametrize("B", [1, 3])
def test_files_written(vae, B, tmp_path):
    """<dir>/<name>.npy: [F,T] when B == 1 (the reference's torch.squeeze), else [B,F,T]; the directory is created."""
    F, T = 37, 5
    maps = torch.rand(9, B, F, T, generator=torch.Generator().manual_seed(B))
    out = tmp_path / "deep" / "maps"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)              # without matplotlib: one warning, .npy only
        vae._write_att_maps(out, maps)
    for l, name in enumerate(LADiffVae.att_map_names):
        got = np.load(out / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == ((F, T) if B == 1 else (B, F, T))
        assert np.array_equal(got.reshape(B, F, T), maps[l].numpy())
    assert sorted(f for f in os.listdir(out) if f.endswith(".npy")) == sorted(n + ".npy" for n in LADiffVae.att_map_names)


@pytest.mark.parametrize("B", [1, 2])
def test_heat_maps_written(vae, B, tmp_path):
    pytest.importorskip("matplotlib")
    maps = torch.rand(9, B, 20, 5, generator=torch.Generator().manual_seed(7))
    vae._write_att_maps(str(tmp_path), maps)
    want = [n + ".png" for n in LADiffVae.att_map_names] if B == 1 else \
        [f"{n}_b{k}.png" for n in LADiffVae.att_map_names for k in range(B)]
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".png")) == sorted(want)
    for f in want:
        with open(tmp_path / f, "rb") as fh:
            assert fh.read(8) == b"\x89PNG\r\n\x1a\n"


def test_without_matplotlib_only_npy_and_one_warning(vae, tmp_path, monkeypatch):
    import builtins
    real = builtins.__import__

    def no_matplotlib(name, *a, **k):
        if name == "matplotlib" or name.startswith("matplotlib."):
            raise ImportError("no matplotlib")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_matplotlib)
    with pytest.warns(RuntimeWarning) as rec:
        vae._write_att_maps(tmp_path, torch.rand(9, 2, 8, 5))
    assert len(rec) == 1
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in LADiffVae.att_map_names)
