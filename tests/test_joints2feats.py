"""joints2feats on the CPU: the numpy restatement (tests/joints2feats_ref.py) against features recorded from the reference's own
`process_file` (tests/golden/make_golden_joints2feats.py), the conditions every test case has to meet, the C-ABI declaration and its
host-side refusals, and the argument errors of `Joints2Feats` and `LADIFF.edit(batch["joints"])` - all without a device."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import joints2feats_ref as ref
from conftest import GOLDEN, ROOT
from ladiff_amd import LADIFF, DDIMScheduler, Joints2Feats, LADiffDenoiser, LADiffVae, _lib
from ladiff_amd.joints2feats import offsets_of_pose
from test_abi import ABL, DEN_KW, VAE_KW

GOLDEN_L = (2, 3, 40, 82, 197)
ALL_L = (2, 3, 40, 82, 162, 197, 256)
ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -4


@pytest.fixture(scope="module")
def g():
    with np.load(os.path.join(GOLDEN, "joints2feats_humanml.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("tag", ["tgt", "raw"])
@pytest.mark.parametrize("L", GOLDEN_L)
def test_restatement_equals_the_reference(g, L, tag):
    """<= 1e-9 in every column (a missed float32 cast shows as >= 1e-8), contacts exactly.  L = 3 pins the frame-axis cross products
    of qbetween's `torch.cross` without a dim; "tgt" the uniform-skeleton step, whose general rotations show torch.cross's fused rounding."""
    x = g[f"x_{L}"]
    assert x.dtype == np.float64 and np.array_equal(x, ref.motion(L, ref.CASE_SEEDS[L]))          # the generator is the recorded input
    got = ref.process_file(x, ref.FEET_THRE, g["tgt_offsets"] if tag == "tgt" else None)
    want = g[f"feats_{tag}_{L}"].astype(np.float64)
    assert got.shape == want.shape == (L - 1, 263)
    assert np.abs(got - want).max() <= 1e-9
    assert np.array_equal(got[:, ref.CONTACT_COLS], want[:, ref.CONTACT_COLS])
    assert set(np.unique(want[:, ref.CONTACT_COLS])) <= {0.0, 1.0}


def test_golden_target_offsets_are_the_target_poses(g):
    assert np.array_equal(ref.get_offsets_joints(g["target_pose"]), g["tgt_offsets"])
    assert np.array_equal(offsets_of_pose(g["target_pose"]).numpy(), g["tgt_offsets"])             # Joints2Feats(target_pose=...)
    assert np.array_equal(ref.get_offsets_joints(ref.target_pose()), g["tgt_offsets"])


def test_the_two_unpackings_differ():
    """process_file's initial facing ADDS hip and shoulder span, the inverse kinematics takes their difference: swapping the hips of
    the input flips neither the facing's sign nor leaves the features alone."""
    x = ref.motion(40, 1)
    a = ref.process_file(x)
    y = x.copy()
    y[:, [1, 2]] = y[:, [2, 1]]
    assert np.abs(ref.process_file(y)[:, 67:193] - a[:, 67:193]).max() > 1e-2


@pytest.mark.parametrize("with_target", [False, True])
@pytest.mark.parametrize("L", ALL_L)
def test_cases_meet_the_conditions(L, with_target):
    x, tgt = ref.case(L, with_target)
    w, margin, s32 = ref.conditioning(x, ref.FEET_THRE, tgt)
    assert w >= ref.W_MIN and margin >= ref.MARGIN_MIN and s32 <= ref.S32_MAX, (w, margin, s32)
    f64, f32 = ref.process_file(x, tgt_offsets=tgt), ref.process_file(x, tgt_offsets=tgt, dtype=np.float32)
    assert np.array_equal(f64[:, ref.CONTACT_COLS], f32[:, ref.CONTACT_COLS])                    # no contact flips in float32
    if L >= 40:
        assert 0.2 < f64[:, ref.CONTACT_COLS].mean() < 0.8                                        # both values occur


def test_generator_is_human_like():
    x = ref.motion(197, 1)
    hips, shoulders = np.linalg.norm(x[:, 1] - x[:, 2], axis=-1), np.linalg.norm(x[:, 16] - x[:, 17], axis=-1)
    assert (shoulders >= 2 * hips).all()
    fwd = np.cross([0, 1, 0], x[:, 17] - x[:, 16])                                                # right - left shoulder: -x when facing +z
    heading = np.arctan2(fwd[:, 0], fwd[:, 2])
    assert abs(heading[0]) <= 0.4 + 0.1 and np.abs(np.diff(heading)).max() < 0.05                 # +-0.4 rad plus the torso twist; a slow turn


def test_gaussian_weights_are_scipys():
    w, radius = ref.gaussian_weights(20)
    assert radius == 80 and len(w) == 161 and abs(w.sum() - 1) < 1e-15 and np.array_equal(w, w[::-1])
    assert np.allclose(w / w[80], np.exp(-np.arange(-80, 81) ** 2 / 800.0), rtol=1e-14)
    ndimage = pytest.importorskip("scipy.ndimage")
    a = np.random.default_rng(0).standard_normal((50, 3))
    assert np.abs(ref.gaussian_filter1d_nearest(a, 20) - ndimage.gaussian_filter1d(a, 20, axis=0, mode="nearest")).max() < 1e-14


# ------------------------------------------------------------------------------------------------ C ABI
def test_entry_is_declared_exported_bound_and_refuses_on_the_host():
    src = open(os.path.join(ROOT, "include", "ladiff_hip.h")).read()
    decl = re.search(r"LADIFF_API int ladiff_joints2feats\(([^)]*)\)", re.sub(r"\s+", " ", src))
    assert decl is not None
    assert [a.strip() for a in decl.group(1).split(",")] == [
        "const float* joints", "const int32_t* h_lengths", "int B", "int L", "int njoints", "const float* target_offsets", "float feet_thre",
        "const float* mean", "const float* std", "float* feats", "ladiff_stream_t stream"]
    for needle in ("motion_process.py:169-351", "HumanML3D.py:50-55", "skeleton.py:43-147", "LADIFF_ERR_UNSUPPORTED"):
        assert needle in src, needle
    assert "ladiff_joints2feats" in _lib.EXPORTS
    from ladiff_amd import build
    assert "joints2feats.hip" in build.SOURCES
    build.build()
    lib = _lib.lib()
    assert lib.ladiff_version() == 6

    def lens(*v):
        return ctypes.cast((ctypes.c_int32 * len(v))(*v), ctypes.c_void_p)

    # the device pointers (16 = an aligned non-NULL address) are never followed: every refusal is answered before any GPU work
    def call(B=2, L=8, J=22, h=None, joints=16, tgt=None, thre=0.002, mean=None, std=None, feats=16):
        return lib.ladiff_joints2feats(joints, h if h is not None else lens(8, 8), B, L, J, tgt, thre, mean, std, feats, None)

    assert call(B=0) == 0 and call(B=-1) == ERR_ARG
    assert call(J=21) == ERR_UNSUPPORTED and call(J=23) == ERR_UNSUPPORTED and call(J=21, B=0) == ERR_UNSUPPORTED
    assert call(L=1, h=lens(1, 1)) == ERR_SHAPE and call(L=257, h=lens(8, 8)) == ERR_SHAPE
    assert call(h=lens(8, 1)) == ERR_SHAPE and call(h=lens(9, 8)) == ERR_SHAPE
    assert call(thre=0.0) == ERR_ARG and call(thre=-1.0) == ERR_ARG
    assert call(mean=16) == ERR_ARG and call(std=16) == ERR_ARG
    assert call(joints=None) == ERR_ARG and call(feats=None) == ERR_ARG
    assert lib.ladiff_joints2feats(16, None, 2, 8, 22, None, 0.002, None, None, 16, None) == ERR_ARG
    for kw in (dict(joints=18), dict(feats=18), dict(tgt=18), dict(mean=18, std=16), dict(mean=16, std=18)):
        assert call(**kw) == ERR_SHAPE, kw


# ------------------------------------------------------------------------------------------------ Python
def test_joints2feats_argument_errors():
    mean, std = np.zeros(263, dtype=np.float32), np.ones(263, dtype=np.float32)
    with pytest.raises(ValueError, match="HumanML3D"):
        Joints2Feats(njoints=21)
    with pytest.raises(ValueError, match="together"):
        Joints2Feats(mean=mean)
    with pytest.raises(ValueError, match="feet_thre"):
        Joints2Feats(feet_thre=0.0)
    with pytest.raises(ValueError, match="not both"):
        Joints2Feats(target_offsets=np.zeros((22, 3)), target_pose=np.zeros((22, 3)))
    with pytest.raises(ValueError, match=r"\[22, 3\]"):
        Joints2Feats(target_offsets=np.zeros((21, 3)))
    with pytest.raises(ValueError, match=r"\[263\]"):
        Joints2Feats(mean=np.zeros(251), std=np.ones(251))
    raw, full = Joints2Feats(), Joints2Feats(mean, std)
    with pytest.raises(_lib.LadiffHipError, match="CPU tensor"):
        raw(torch.zeros(8, 22, 3))
    with pytest.raises(_lib.LadiffHipError, match="CPU tensor"):
        full(torch.zeros(2, 8, 22, 3), [8, 8], normalize=True)
    with pytest.raises(ValueError, match="statistics"):
        raw.check((8, 22, 3), None, normalize=True)
    for shape, lengths, msg in (((8, 21, 3), None, "joints must be"), ((1, 22, 3), None, "2 .. 256 frames"), ((257, 22, 3), None, "2 .. 256"),
                                ((2, 8, 22, 3), [8], "1 lengths for 2"), ((2, 8, 22, 3), [8, 1], "lengths must lie"),
                                ((2, 8, 22, 3), [9, 8], "lengths must lie")):
        with pytest.raises(ValueError, match=msg):
            full.check(shape, lengths)
    assert full.check((2, 8, 22, 3), None) == (2, 8, [8, 8]) and full.check((5, 22, 3), None, True) == (1, 5, [5])
    assert full.check((0, 8, 22, 3), []) == (0, 8, [])
    dm = SimpleNamespace(hparams=SimpleNamespace(mean=mean, std=std), njoints=22)
    assert torch.equal(Joints2Feats.from_datamodule(dm).std, torch.ones(263))
    assert Joints2Feats.from_datamodule(SimpleNamespace(mean=np.zeros(251), std=np.ones(251), njoints=21)) is None      # KIT: not built
    assert Joints2Feats.from_datamodule(SimpleNamespace(njoints=22)) is None


def _pipe(datamodule):
    return LADIFF(denoiser=LADiffDenoiser(ABL, **DEN_KW), vae=LADiffVae(ABL, **VAE_KW), datamodule=datamodule,
                  scheduler=DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                          set_alpha_to_one=False, steps_offset=1, clip_sample=False),
                  guidance_scale=7.5, num_inference_timesteps=6, eta=0.0, max_it=5, text_encoder=lambda t: torch.zeros(len(t), 1, 768))


def test_edit_refuses_a_bad_joints_source_on_the_host():
    """Every tensor here is a CPU tensor: an accepted source would end in LadiffHipError at the first device call."""
    dm = SimpleNamespace(hparams=SimpleNamespace(mean=np.zeros(263, dtype=np.float32), std=np.ones(263, dtype=np.float32)), njoints=22,
                         feats2joints=lambda f: f)
    pipe, lens = _pipe(dm), [40, 40]
    assert pipe.joints2feats_device is not None and pipe.joints2feats_device.mean is not None
    joints = torch.zeros(2, 41, 22, 3)
    base = {"text": ["a", "b"], "length": lens}
    for extra, kw in (({"joints": joints, "motion": torch.zeros(2, 40, 263)}, {}), ({"joints": joints}, {"latents": torch.zeros(5, 2, 256)}),
                      ({}, {})):
        with pytest.raises(ValueError, match="exactly one source"):
            pipe.edit({**base, **extra}, 0.5, **kw)
    with pytest.raises(ValueError, match="joints"):
        pipe.edit({**base}, 0.5)                                                                   # the message names the third source
    with pytest.raises(NotImplementedError, match="encode handles up to"):
        pipe.edit({**base, "joints": torch.zeros(2, 216, 22, 3)}, 0.5)                             # 215 feature frames + 2 x 5 > 224
    with pytest.raises(ValueError, match="lengths must lie"):
        pipe.edit({**base, "joints": joints, "source_length": [41, 42]}, 0.5)
    with pytest.raises(ValueError, match="3 joint sources for 2 prompts"):
        pipe.edit({**base, "joints": [torch.zeros(41, 22, 3)] * 3}, 0.5)
    with pytest.raises(ValueError, match="joints must be"):
        pipe.edit({**base, "joints": torch.zeros(2, 41, 21, 3)}, 0.5)
    with pytest.raises(ValueError, match="padded"):
        pipe.edit({**base, "joints": torch.zeros(41, 22, 3)}, 0.5)
    with pytest.raises(_lib.LadiffHipError):                                                       # a good source reaches the device check
        pipe.edit({**base, "joints": joints}, 0.5)
    with pytest.raises(_lib.LadiffHipError):
        pipe.forward_motion_style_transfer({**base, "joints": [torch.zeros(41, 22, 3), torch.zeros(30, 22, 3)]})
    bare = _pipe(SimpleNamespace(feats2joints=lambda f: f))                                        # no statistics: no device joints2feats
    with pytest.raises(RuntimeError, match="joints2feats_device"):
        bare.edit({**base, "joints": joints}, 0.5)
