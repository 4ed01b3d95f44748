"""The renderer on the GPU (csrc/render.hip) against the float64 restatement of its image model (tests/render_ref.py).

The gate is the construction of test_gpu_joints2feats.py: 4 x max(e32, s32), both CPU figures computed here - e32 the restatement's
float32 run against its float64 run, s32 the float64 restatement on float32-rounded joints against itself on the float64 joints.  Every
case prints its error beside its gate (profiles/render/ keeps one run's lines).  uint8 images are held to one level of
floor(255 ref64 + 0.5) at every byte.  Sizes are W x H: 64 x 48 is whole 64 x 16 tiles, 68 x 36 has partial tiles both ways."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import render_ref as ref
from ladiff_amd import LADIFF, DDIMScheduler, LADiffDenoiser, LADiffVae, MotionRenderer, _lib, synthetic as syn
from test_abi import ABL, DEN_KW, VAE_KW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CASES = {}


def eye(st, H, W):
    return ref.camera(st, H, W, st["dist"], np.float64)


def build_case(name):
    """(joints float64 [B,L,J,3], lengths, H, W, style overrides) of a frames case."""
    if name == "whole_tiles":                    # W x H = 64 x 48
        return np.stack([ref.motion(2, 22, seed=1)]), [2], 48, 64, {}
    if name == "partial_tiles_kit":              # W x H = 68 x 36, the 21-joint skeleton
        return np.stack([ref.motion(2, 21, seed=2)]), [2], 36, 68, {}
    if name == "256":
        return np.stack([ref.motion(3, 22, seed=3), ref.motion(3, 22, seed=4, travel=2.0)]), [3, 2], 256, 256, {}
    if name == "kit_256x128":
        return np.stack([ref.motion(2, 21, seed=5)]), [2], 128, 256, {}
    if name == "crosses_the_border":             # a close camera: the figure is larger than the image - culled, partly covered and empty tiles
        return np.stack([ref.motion(2, 22, seed=6)]), [2], 96, 256, dict(dist=1.4, target_height=1.2)
    if name == "pose_off_image":                 # frame 1 floats 10 units above the floor that frame 0 sets: only ground and background show
        x = ref.motion(2, 22, seed=7, travel=2.0)
        x[1, :, 1] += 10.0
        return x[None], [2], 96, 128, {}
    if name == "joint_behind_the_eye":           # the left wrist 1.5 units behind the camera: its bone is skipped, the rest is intact
        x = ref.motion(2, 22, seed=8)
        cam = eye(ref.style(96), 96, 128)
        behind = cam["E"] - 1.5 * cam["f"]          # where the drawn point has to be: 2.2 above the floor, so the floor stays the feet's
        x[1, 20] = behind + np.array([x[1, 0, 0], x[:, :, 1].min(), x[1, 0, 2]])
        return x[None], [2], 96, 128, {}
    if name == "horizon_inside":                 # a low camera over a long walk: the ground runs towards a horizon in the upper half
        return np.stack([ref.motion(3, 22, seed=9, travel=8.0)]), [3], 96, 128, dict(elev_deg=3.0, ground_alpha=0.9)
    if name == "coincident_joints":
        x = ref.motion(2, 22, seed=10)
        x[:, 20] = x[:, 18]
        x[1, 7] = x[1, 4]
        return x[None], [2], 48, 64, {}
    raise KeyError(name)


FRAME_CASES = ("whole_tiles", "partial_tiles_kit", "256", "kit_256x128", "crosses_the_border", "pose_off_image", "joint_behind_the_eye",
               "horizon_inside", "coincident_joints")


def gate_of(run, x):
    """(float64 result, gate, e32, s32) of `run(joints, dtype)`; CPU only."""
    want = run(x, np.float64)
    e32 = float(np.abs(run(x, np.float32).astype(np.float64) - want).max())
    s32 = float(np.abs(run(x.astype(np.float32).astype(np.float64), np.float64) - want).max())
    return want, 4 * max(e32, s32), e32, s32


def case(name):
    if name not in _CASES:
        x, lengths, H, W, over = build_case(name)
        st = ref.style(H, **over)
        run = lambda xx, dt: np.stack([ref.render_frames(xx[b], lengths[b], H, W, st, dtype=dt) for b in range(len(lengths))])
        _CASES[name] = (x, lengths, H, W, st) + gate_of(run, x)
    return _CASES[name]


def dev32(x):
    return torch.from_numpy(np.asarray(x)).to(torch.float32).to(DEV)


def renderer(x, H, W, st):
    """The restatement's style goes in as keywords: same names, and by test_render.py the same defaults."""
    return MotionRenderer(njoints=x.shape[-2], size=(H, W), **st)


@pytest.mark.parametrize("name", FRAME_CASES)
def test_float_images_match_the_restatement(name):
    x, lengths, H, W, st, want, gate, e32, s32 = case(name)
    got = renderer(x, H, W, st)(dev32(x), lengths, dtype=torch.float32).cpu().double().numpy()
    assert got.shape == want.shape == (len(lengths), x.shape[1], H, W, 3)
    err = float(np.abs(got - want).max())
    print(f"{name} {W}x{H}: max|kernel - fp64 restatement| = {err:.2e}, gate {gate:.2e} = 4 x max(e32 {e32:.1e}, s32 {s32:.1e})")
    assert 0 < gate < 1e-2                                              # the gate is a rounding figure, not a tolerance someone chose
    assert np.isfinite(got).all() and err <= gate
    # what each case is there for.  Background and ground are greys, the chains are not: `figure` marks the pixels a bone reaches
    bg, figure = np.asarray(st["background"]), want.max(axis=-1) - want.min(axis=-1) > 1e-3
    ground = ~figure & (np.abs(want - bg).max(axis=-1) > 1e-3)
    if name == "pose_off_image":
        assert figure[0, 0].any() and not figure[0, 1].any() and ground[0, 1].any() and (np.abs(want[0, 1] - 0.75).max(axis=-1) < 1e-9).any()
    if name == "crosses_the_border":
        tiles = figure[0, 0].reshape(H // 16, 16, W // 64, 64).any(axis=(1, 3))
        assert tiles.any() and not tiles.all() and figure[0, 0][-1].any()
    if name == "joint_behind_the_eye":
        P = x[0, 1] - np.array([x[0, 1, 0, 0], x[0].min(axis=(0, 1))[1], x[0, 1, 0, 2]])
        zc = ref.project(P, eye(st, H, W), np.float64)[2]
        assert zc[20] < -1.0 and (np.delete(zc, 20) > 1.0).all() and figure[0, 1].any()
    if name == "256":
        assert np.array_equal(got[1, 2], np.broadcast_to(bg, (H, W, 3)))  # image 2 of the motion of length 2
    if name == "horizon_inside":
        rows = np.where(ground[0, 2].any(axis=1))[0]                     # the last frame: the walked ground lies behind the figure
        assert H // 4 < rows.min() < 3 * H // 4                          # sky above it, inside the image


@pytest.mark.parametrize("name", ["256", "crosses_the_border", "partial_tiles_kit"])
def test_uint8_images_are_within_one_level(name):
    x, lengths, H, W, st, want = case(name)[:6]
    got = renderer(x, H, W, st)(dev32(x), lengths).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape
    diff = np.abs(got.astype(np.int32) - ref.to_uint8(want).astype(np.int32))
    print(f"{name}: uint8 max level difference {diff.max()}, bytes that differ {int((diff > 0).sum())} of {diff.size}")
    assert diff.max() <= 1


def test_ragged_batch_is_each_motion_alone():
    """Lengths [1, 5, 3] in L = 5 through the C ABI: every element is written (NaN-filled float output; two different sentinel bytes
    for uint8), images t >= len are exactly the background, and each motion's images are the bits of that motion launched alone."""
    lens, L, H, W = [1, 5, 3], 5, 36, 68
    r = MotionRenderer(size=(H, W))
    batch = torch.full((3, L, 22, 3), float("nan"))                       # frames past a motion's length are never read
    for b, l in enumerate(lens):
        batch[b, :l] = torch.from_numpy(ref.motion(l, 22, seed=20 + b, travel=1.0 + b)).float()
    x = batch.to(DEV)
    lib, p, h_len = _lib.lib(), r.params(), (ctypes.c_int32 * 3)(*lens)
    nbytes = lib.ladiff_render_workspace_bytes(3)
    ws = _lib.workspace(nbytes, DEV)

    def run(out, is_float):
        _lib.check(lib.ladiff_render_motion(_lib.ptr(x), h_len, 3, L, 22, ctypes.byref(p), 0, 1, H, W, out.data_ptr(), is_float, _lib.ptr(ws),
                                            nbytes, _lib.stream_ptr()))
        return out.cpu()
    as_float = run(torch.full((3, L, H, W, 3), float("nan"), device=DEV), 1)
    assert torch.isfinite(as_float).all()
    as_bytes = run(torch.full((3, L, H, W, 3), 0xAB, dtype=torch.uint8, device=DEV), 0)
    assert torch.equal(as_bytes, run(torch.full((3, L, H, W, 3), 0x54, dtype=torch.uint8, device=DEV), 0))
    assert torch.equal(as_float, r(x, lens, dtype=torch.float32).cpu()) and torch.equal(as_bytes, r(x, lens).cpu())      # the class is this call
    for b, l in enumerate(lens):
        assert (as_float[b, l:] == 1.0).all() and (as_bytes[b, l:] == 255).all()
        alone = batch[b, :l].contiguous().to(DEV)
        assert torch.equal(as_float[b, :l], r(alone, dtype=torch.float32).cpu()), b
        assert torch.equal(as_bytes[b, :l], r(alone).cpu()), b
        assert (as_bytes[b, :l] != 255).any()
    strips = r.strip(x, lens, dtype=torch.float32).cpu()
    for b, l in enumerate(lens):
        assert torch.equal(strips[b], r.strip(batch[b, :l].contiguous().to(DEV), dtype=torch.float32).cpu()), b


@pytest.mark.parametrize("length,travel", [(1, 1.0), (2, 1.0), (40, 1.0), (40, 7.0)])
def test_strip_matches_the_restatement(length, travel):
    H, W, n_poses = 96, 128, 8
    st = ref.style(H)
    x = ref.motion(length, 22, seed=30 + length, travel=travel)
    mins, maxs = ref.scene(x, length)
    fit = float(ref.strip_distance(st, mins, maxs, np.float64)) / st["dist"]
    assert (fit > 1.5) if travel > 3 else (fit == 1.0)                    # the far walk is the case whose camera backs off
    want, gate, e32, s32 = gate_of(lambda xx, dt: ref.render_strip(xx, length, n_poses, H, W, st, dtype=dt), x)
    r = renderer(x, H, W, st)
    got = r.strip(dev32(x), n_poses=n_poses, dtype=torch.float32).cpu().double().numpy()
    err = float(np.abs(got - want).max())
    print(f"strip len={length} travel={travel} (distance x {fit:.2f}): max|kernel - fp64 restatement| = {err:.2e}, gate {gate:.2e} = 4 x "
          f"max(e32 {e32:.1e}, s32 {s32:.1e})")
    assert got.shape == (H, W, 3) and 0 < gate < 1e-2 and err <= gate
    diff = np.abs(r.strip(dev32(x), n_poses=n_poses).cpu().numpy().astype(np.int32) - ref.to_uint8(want).astype(np.int32))
    assert diff.max() <= 1


def test_frame_stride_gives_every_third_image():
    x = dev32(np.stack([ref.motion(8, 22, seed=40), ref.motion(8, 22, seed=41)]))
    r = MotionRenderer(size=(48, 64))
    for dtype in (torch.uint8, torch.float32):
        full, third = r(x, [8, 5], dtype=dtype), r(x, [8, 5], dtype=dtype, frame_stride=3)
        assert third.shape == (2, 3, 48, 64, 3) and torch.equal(third, full[:, ::3])
    assert r(x[0], frame_stride=8).shape == (1, 48, 64, 3)


def make_model():
    den = LADiffDenoiser(ABL, **DEN_KW); den.load_state_dict(syn.denoiser_weights(), strict=True)
    vae = LADiffVae(ABL, **VAE_KW); vae.load_state_dict(syn.vae_weights(263), strict=True)
    gen = torch.Generator().manual_seed(97)
    enc_out = torch.randn(4, 1, 768, generator=gen)
    mean, std = 0.1 * torch.randn(263, generator=gen), 0.5 + torch.rand(263, generator=gen)
    dm = SimpleNamespace(feats2joints=None, hparams=SimpleNamespace(mean=mean.numpy(), std=std.numpy()), njoints=22)
    return LADIFF(None, dm, denoiser=den.to(DEV).eval(), vae=vae.to(DEV).eval(), text_encoder=lambda texts: enc_out.to(DEV), guidance_scale=7.5,
                  num_inference_timesteps=6, eta=0.0, max_it=5,
                  scheduler=DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                          set_alpha_to_one=False, steps_offset=1, clip_sample=False))


def test_pipeline_renders_animates_and_previews(tmp_path):
    model = make_model()
    batch = {"text": ["a person walks", "a person jumps"], "length": [24, 60], "seed": [11, 12]}
    joints = model.forward(batch)
    assert [tuple(j.shape) for j in joints] == [(24, 22, 3), (60, 22, 3)]
    model.renderer = MotionRenderer(22, size=(64, 64))
    frames = model.render(joints)
    assert frames.shape == (2, 60, 64, 64, 3) and frames.dtype == torch.uint8 and frames.is_cuda
    padded = torch.zeros(2, 60, 22, 3)
    padded[0, :24], padded[1] = joints[0], joints[1]
    assert torch.equal(frames, model.render(padded, [24, 60])) and torch.equal(frames, model.renderer(padded.to(DEV), [24, 60]))
    assert (frames[0, 24:] == 255).all() and (frames[0, :24] != 255).any()
    strips = model.strip(joints, n_poses=4)
    assert strips.shape == (2, 64, 64, 3) and torch.equal(strips, model.renderer.strip(padded.to(DEV), [24, 60], n_poses=4))

    back = model.animate(batch, tmp_path / "out")
    assert all(torch.equal(a, b) for a, b in zip(back, joints))
    assert sorted(os.listdir(tmp_path / "out")) == ["0.gif", "0.txt", "0_strip.png", "1.gif", "1.txt", "1_strip.png"]
    assert (tmp_path / "out" / "1.txt").read_text() == "a person jumps\n60\n"
    Image = pytest.importorskip("PIL.Image")
    for i, l in enumerate(batch["length"]):
        with Image.open(tmp_path / "out" / f"{i}.gif") as im:          # the writer folds identical neighbours into one longer frame
            shown_ms = 0
            for k in range(im.n_frames):
                im.seek(k)
                shown_ms += im.info["duration"]
            assert im.size == (64, 64) and 1 < im.n_frames <= l and shown_ms == 50 * l
        with Image.open(tmp_path / "out" / f"{i}_strip.png") as im:
            assert np.array_equal(np.asarray(im.convert("RGB")), model.strip(joints)[i].cpu().numpy())
    model.animate(batch, tmp_path / "bare", strip=False)
    assert sorted(os.listdir(tmp_path / "bare")) == ["0.gif", "0.txt", "1.gif", "1.txt"]

    plain = model.preview(batch, steps=[0, 3, 5])
    shown = model.preview(batch, steps=[0, 3, 5], render="strip")
    assert len(plain) == 2 and len(shown) == 3                             # without `render`: what it returned before
    for a, b in zip(plain[0], shown[0]):
        assert torch.equal(a, b)
    for ka, kb in zip(plain[1], shown[1]):
        assert all(torch.equal(a, b) for a, b in zip(ka, kb))
    pictures = shown[2]
    assert len(pictures) == 2 and all(p.shape == (3 * 64, 64, 3) and p.dtype == torch.uint8 and not p.is_cuda for p in pictures)
    for b in range(2):
        for k in range(3):
            assert torch.equal(pictures[b][k * 64:(k + 1) * 64], model.strip([shown[1][k][b]])[0].cpu())
    with pytest.raises(ValueError):
        model.preview(batch, render="frames")
