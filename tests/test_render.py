"""The renderer without a GPU: facts of the image model's restatement (tests/render_ref.py, written from include/ladiff_hip.h) that hold by
construction, and every host-side refusal of `MotionRenderer`, `save_animation` and `ladiff_render_motion`."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import render_ref as ref
from ladiff_amd import MotionRenderer, _lib, render, save_animation

H, W = 96, 128


def test_the_restated_tables_are_the_package_tables():
    assert ref.CHAINS == render.CHAINS
    assert ref.CHAIN_RGB == tuple(render.rgb(c) for c in render.CHAIN_COLORS)
    st, r = ref.style(H), MotionRenderer(size=(H, W)).style
    assert {k: tuple(v) if isinstance(v, (tuple, list)) else v for k, v in st.items()} == r
    assert len(ref.bones(22)) == 21 and len(ref.bones(21)) == 20


@pytest.mark.parametrize("J", [22, 21])
def test_the_pixel_at_a_projected_joint_has_its_chains_colour(J):
    """Line width 4: a pixel whose centre is within 0.71 of the joint is fully covered.  The last joint of each chain, on a standing
    figure whose limbs are apart: nothing drawn later reaches it."""
    st = ref.style(H, line_width=4.0)
    x = ref.standing_pose(J)[None]
    img = ref.render_frames(x, 1, H, W, st)[0]
    cam = ref.camera(st, H, W, st["dist"], np.float64)
    mins, _ = ref.scene(x, 1)
    sx, sy, zc = ref.project(x[0] - np.array([x[0, 0, 0], mins[1], x[0, 0, 2]]), cam, np.float64)
    for k, chain in enumerate(ref.CHAINS[J]):
        j = chain[-1]
        assert zc[j] > st["near"] and 0 <= sx[j] < W and 0 <= sy[j] < H
        assert np.allclose(img[int(sy[j]), int(sx[j])], st["chain_colors"][k], atol=1e-12), (J, k)
    assert np.array_equal(img[0, 0], st["background"]) and np.array_equal(img[0, W - 1], st["background"])      # far corners: sky


def test_a_ray_into_the_ground_rectangle_gives_half_white_half_grey():
    st = ref.style(H)
    x = ref.motion(9, travel=2.0)
    t = 4
    img = ref.render_frames(x, 9, H, W, st)[t]
    cam = ref.camera(st, H, W, st["dist"], np.float64)
    mins, maxs = ref.scene(x, 9)
    rx, rz = x[t, 0, 0], x[t, 0, 2]
    cov = ref.ground_coverage(cam, (mins[0] - rx, maxs[0] - rx, mins[2] - rz, maxs[2] - rz), np.float64)
    sx, sy, _ = ref.project(x[t] - np.array([rx, mins[1], rz]), cam, np.float64)
    px, py = ref.pixel_centres(H, W, np.float64)
    away = np.min(np.hypot(px[None] - sx[:, None, None], py[None] - sy[:, None, None]), axis=0)
    away[cov < 1.0] = -1.0
    i, j = np.unravel_index(np.argmax(away), away.shape)
    assert away[i, j] > 10.0                                          # ten pixels from every joint: no bone (<= 6 pixels long here) reaches it
    assert np.array_equal(img[i, j], [0.75, 0.75, 0.75])
    assert (cov == 0).any() and ((cov > 0) & (cov < 1)).any()          # the rectangle is bounded: it has an edge inside the image


def test_a_mirrored_pose_seen_from_the_front_gives_the_mirrored_image():
    """az = 0: x -> -x is the image's left-right flip.  One colour for all chains, since mirroring swaps the left and right limbs."""
    st = ref.style(H, azim_deg=0.0, chain_colors=(ref.CHAIN_RGB[0],) * 5)
    x = ref.motion(3, seed=3)
    m = x * np.array([-1.0, 1.0, 1.0])
    a, b = ref.render_frames(x, 3, H, W, st), ref.render_frames(m, 3, H, W, st)
    assert np.abs(a[:, :, ::-1] - b).max() < 1e-9
    assert np.abs(a - b).max() > 0.1                                  # and the pose is not symmetric itself


def test_strip_pose_indices():
    for length in (1, 2, 7, 196):
        for n_poses in (1, 2, 8):
            idx = ref.strip_indices(length, n_poses)
            assert len(idx) == min(n_poses, length) and idx[0] == 0
            assert all(0 <= t < length for t in idx) and all(a < b for a, b in zip(idx, idx[1:])), (length, n_poses, idx)
            if len(idx) > 1:
                assert idx[-1] == length - 1
    assert ref.strip_indices(196, 8) == [0, 28, 56, 84, 111, 139, 167, 195]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_zero_length_bone_is_a_dot_and_nothing_is_nan(dtype):
    st = ref.style(H, line_width=4.0)
    x = ref.standing_pose()[None].copy()
    x[0, 20] = x[0, 18]                                               # the last bone of the last chain has no length
    with np.errstate(all="raise"):
        img = ref.render_frames(x, 1, H, W, st, dtype=dtype)
        strip = ref.render_strip(np.repeat(x, 3, axis=0), 3, 8, H, W, st, dtype=dtype)      # no extent at all in x and z travel
    assert img.dtype == dtype and np.isfinite(img).all() and np.isfinite(strip).all()
    assert img.min() >= 0 and img.max() <= 1
    cov = ref.bone_coverage((10.3, 20.6), (10.3, 20.6), H, W, 4.0, dtype)
    assert cov[20, 10] == 1 and cov.sum() > 4 and cov[30, 10] == 0 and np.isfinite(cov).all()


# ---------------------------------------------------------------- host checks
def test_constructor_and_check_refuse():
    for kw in (dict(njoints=20), dict(size=(64, 66)), dict(size=(8, 64)), dict(size=(64, 2048)), dict(elev_deg=90), dict(dist=0), dict(focal=-1),
               dict(line_width=0), dict(target_height=-2.0), dict(alpha_min=1.5), dict(background=(2, 0, 0)), dict(chain_colors=("#000000",) * 4)):
        with pytest.raises(ValueError):
            MotionRenderer(**kw)
    with pytest.raises(TypeError, match="zoom"):
        MotionRenderer(zoom=2)
    r = MotionRenderer(size=(64, 96))
    assert r.check((5, 22, 3), None) == (1, 5, [5], (1, 5, 64, 96, 3))
    assert r.check((2, 5, 22, 3), [1, 5], frame_stride=2)[3] == (2, 3, 64, 96, 3)
    assert r.check((2, 5, 22, 3), [1, 5], n_poses=8)[3] == (2, 64, 96, 3)
    for shape, lengths, kw in (((5, 21, 3), None, {}), ((5, 22), None, {}), ((2, 257, 22, 3), None, {}), ((2, 0, 22, 3), None, {}),
                               ((2, 5, 22, 3), [5], {}), ((2, 5, 22, 3), [0, 5], {}), ((2, 5, 22, 3), [5, 6], {}),
                               ((2, 5, 22, 3), None, dict(dtype=torch.float16)), ((2, 5, 22, 3), None, dict(frame_stride=0)),
                               ((2, 5, 22, 3), None, dict(n_poses=0))):
        with pytest.raises(ValueError):
            r.check(shape, lengths, **kw)
    assert MotionRenderer(njoints=21).check((3, 21, 3), None)[0] == 1


def test_a_request_above_max_render_bytes_is_refused_by_name():
    r = MotionRenderer(size=(256, 256))
    assert r.max_render_bytes == 8 << 30
    r.check((128, 196, 22, 3), None)                                  # 4.9 GB of uint8: served
    with pytest.raises(ValueError, match="max_render_bytes") as e:
        r.check((128, 196, 22, 3), None, dtype=torch.float32)         # 19.7 GB
    assert "frame_stride" in str(e.value) and "size" in str(e.value)
    r.check((128, 196, 22, 3), None, dtype=torch.float32, frame_stride=3)
    r.max_render_bytes = 1000
    with pytest.raises(ValueError, match="max_render_bytes"):
        r.check((1, 22, 3), None, n_poses=8)


def test_cpu_tensors_raise():
    r = MotionRenderer(size=(64, 64))
    with pytest.raises(_lib.LadiffHipError):
        r(torch.zeros(3, 22, 3))
    with pytest.raises(_lib.LadiffHipError):
        r.strip(torch.zeros(2, 3, 22, 3), [3, 3])
    with pytest.raises(TypeError):
        r(np.zeros((3, 22, 3)))


def test_save_animation_npy_and_refusals(tmp_path, monkeypatch):
    frames = (np.random.default_rng(0).random((4, 16, 20, 3)) * 255).astype(np.uint8)
    p = save_animation(torch.from_numpy(frames), tmp_path / "a.npy")
    assert np.array_equal(np.load(p), frames)
    as_float = np.load(save_animation(frames.astype(np.float32) / 255.0, tmp_path / "b.npy"))
    assert np.array_equal(as_float, frames)                           # floor(255 c + 0.5)
    with pytest.raises(ValueError):
        save_animation(frames, tmp_path / "a.mp4")
    with pytest.raises(ValueError):
        save_animation(frames[..., :2], tmp_path / "a.npy")
    monkeypatch.setitem(sys.modules, "PIL", None)                      # an import of PIL now fails as if it were not installed
    with pytest.raises(RuntimeError, match="PIL"):
        save_animation(frames, tmp_path / "a.gif")
    save_animation(frames, tmp_path / "c.npy")


def test_save_animation_round_trips_a_gif_and_an_apng(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    palette = np.array([[255, 255, 255], [191, 191, 191], [221, 90, 55], [214, 158, 0]], dtype=np.uint8)
    frames = palette[np.random.default_rng(1).integers(0, 4, size=(5, 16, 20))]
    for name in ("a.gif", "a.png"):
        with Image.open(save_animation(frames, tmp_path / name, fps=20)) as im:
            assert im.n_frames == 5 and im.size == (20, 16)
            for k in range(5):
                im.seek(k)
                assert np.array_equal(np.asarray(im.convert("RGB")), frames[k]), (name, k)
            assert name.endswith(".png") or im.info["duration"] == 50
    with Image.open(save_animation(frames[0], tmp_path / "one.png")) as im:
        assert np.array_equal(np.asarray(im.convert("RGB")), frames[0])


@pytest.fixture(scope="module")
def lib():
    from ladiff_amd import build
    build.build()
    return _lib.lib()


def test_every_error_code_comes_back_before_anything_is_queued(lib):
    """Host code only: the pointers are fakes that are never followed (the pattern of test_graphed_decode_refuses_on_the_host_like_the_
    ragged_one).  No call here has arguments that would pass."""
    ARG, SHAPE, WORKSPACE, UNSUPPORTED = -1, -2, -3, -4
    fake = 0x1000
    q = lib.ladiff_render_workspace_bytes(2)
    assert q > 0 and lib.ladiff_render_workspace_bytes(0) == 0
    assert all(lib.ladiff_render_workspace_bytes(b + 1) >= lib.ladiff_render_workspace_bytes(b) for b in range(300))

    def call(joints=fake, lengths=(3, 5), B=2, L=5, J=22, mode=0, n_poses=8, H=64, W=64, out=fake, is_float=1, ws=fake, ws_bytes=q, params=True,
             frame_stride=1, **style):
        p = MotionRenderer(size=(64, 64)).params(frame_stride)
        for k, v in style.items():
            setattr(p, k, v)
        h = (ctypes.c_int32 * len(lengths))(*lengths) if lengths is not None else None
        return lib.ladiff_render_motion(joints, h, B, L, J, ctypes.byref(p) if params else None, mode, n_poses, H, W, out, is_float, ws, ws_bytes,
                                        None)
    assert call(ws_bytes=q - 1) == WORKSPACE                           # ... so every other argument of the default call is accepted
    assert call(J=20) == UNSUPPORTED and call(J=263) == UNSUPPORTED and call(J=20, B=-1) == UNSUPPORTED
    for kw in (dict(B=-1), dict(joints=None), dict(lengths=None), dict(params=False), dict(out=None), dict(ws=None), dict(mode=2), dict(mode=-1),
               dict(n_poses=0), dict(frame_stride=0), dict(elev_deg=90.0), dict(elev_deg=-90.0), dict(target_height=-1.0), dict(dist=0.0),
               dict(focal=0.0), dict(line_width=0.0), dict(dist=-1.0), dict(near_plane=0.0), dict(ground_alpha=1.5), dict(dist=float("nan"))):
        assert call(**kw) == ARG, kw
    for kw in (dict(L=0), dict(L=257, lengths=(3, 257)), dict(H=8), dict(H=1025), dict(W=12), dict(W=1028), dict(W=66), dict(lengths=(0, 5)),
               dict(lengths=(3, 6)), dict(joints=fake + 2), dict(ws=fake + 1), dict(out=fake + 4), dict(out=fake + 2, is_float=0)):
        assert call(**kw) == SHAPE, kw
    assert call(out=fake + 4, is_float=0, ws_bytes=0) == WORKSPACE      # uint8 images need 4-byte alignment only
    assert call(dist=0.0, L=0, ws_bytes=0) == ARG and call(L=0, ws_bytes=0) == SHAPE      # the order: argument, shape, workspace
    assert call(B=0, joints=None, lengths=None, out=None, ws=None, ws_bytes=0) == 0
