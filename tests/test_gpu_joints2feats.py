"""joints2feats on the GPU (csrc/joints2feats.hip) against the fp64 restatement of the reference's `process_file`
(tests/joints2feats_ref.py, itself pinned to the reference's recorded output in tests/test_joints2feats.py): parity over the lengths at
which the kernel takes another path, ragged batches, the fused normalisation, the input forms and `LADIFF.edit(batch["joints"])`.

Measured on an MI355X, max |kernel - restatement| over the 259 non-contact columns beside its gate 4 x max(e32, s32) (e32: the
restatement's float32 run against its float64 run, s32: the restatement under float32 rounding of its input - both CPU figures):
see DESIGN.md 8 "joints2feats" for the table; contacts were equal in every case."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import joints2feats_ref as ref
from conftest import load_golden
from ladiff_amd import LADIFF, DDIMScheduler, Joints2Feats, LADiffDenoiser, LADiffVae, synthetic as syn
from test_abi import ABL, DEN_KW, VAE_KW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = (2, 3, 40, 82, 162, 197, 256)       # one row; the 3-frame cross products; < radius; radius and full window just inside; HumanML's 196; the limit
GOLDEN_L = (2, 3, 40, 82, 197)
_CASES = {}


def case(L, with_target):
    """(input float64, target offsets, fp64 restatement, gate) of a case, computed once on the CPU; nobody writes into it."""
    key = (L, with_target)
    if key not in _CASES:
        x, tgt = ref.case(L, with_target)
        w, margin, s32 = ref.conditioning(x, ref.FEET_THRE, tgt)
        assert w >= ref.W_MIN and margin >= ref.MARGIN_MIN and s32 <= ref.S32_MAX, (w, margin, s32)
        want = ref.process_file(x, ref.FEET_THRE, tgt)
        e32 = float(np.abs(ref.process_file(x, ref.FEET_THRE, tgt, dtype=np.float32)[:, :259] - want[:, :259]).max())
        _CASES[key] = (x, tgt, want, 4 * max(e32, s32), e32, s32)
    return _CASES[key]


def j2f(tgt=None, **kw):
    return Joints2Feats(target_offsets=tgt, **kw)


def dev32(x):
    return torch.from_numpy(np.asarray(x)).to(torch.float32).to(DEV)


@pytest.mark.parametrize("with_target", [False, True])
@pytest.mark.parametrize("L", LENGTHS)
def test_parity_with_the_fp64_restatement(L, with_target):
    x, tgt, want, gate, e32, s32 = case(L, with_target)
    if L in GOLDEN_L:                                                       # where recorded, the yardstick IS the reference's output
        g = load_golden("joints2feats_humanml")
        assert np.abs(g[f"feats_{'tgt' if with_target else 'raw'}_{L}"].double().numpy() - want).max() <= 1e-9
    got = j2f(tgt)(dev32(x)).cpu().double().numpy()
    assert got.shape == (L - 1, 263)
    err = np.abs(got[:, :259] - want[:, :259]).max()
    col = int(np.abs(got[:, :259] - want[:, :259]).max(axis=0).argmax())
    print(f"L={L} target={with_target}: max|kernel - fp64 restatement| = {err:.2e} (column {col}), gate {gate:.2e} = 4 x max(e32 {e32:.1e}, "
          f"s32 {s32:.1e}); contact mismatches {int((got[:, 259:] != want[:, 259:]).sum())}")
    assert np.array_equal(got[:, ref.CONTACT_COLS], want[:, ref.CONTACT_COLS])
    assert err <= gate


@pytest.mark.parametrize("with_target", [False, True])
def test_ragged_batch_is_each_motion_alone(with_target):
    """Lengths [2, 40, 197] in one launch, through the C ABI into a NaN-filled buffer (a row the kernel skipped would stay NaN): per motion
    the bits of that motion launched alone, zeros from row L_b - 1 on."""
    import ctypes
    from ladiff_amd import _lib
    lens = [2, 40, 197]
    tgt = case(40, with_target)[1]
    batch = torch.zeros(3, 197, 22, 3)
    for b, l in enumerate(lens):
        batch[b, :l] = torch.from_numpy(case(l, with_target)[0]).float()
        batch[b, l:] = float("nan")                                         # frames past a motion's length are never read
    x, d_tgt = batch.to(DEV), (None if tgt is None else dev32(tgt))
    out = torch.full((3, 196, 263), float("nan"), device=DEV)
    _lib.check(_lib.lib().ladiff_joints2feats(_lib.ptr(x), (ctypes.c_int32 * 3)(*lens), 3, 197, 22, _lib.ptr(d_tgt), 0.002, None, None,
                                              _lib.ptr(out), _lib.stream_ptr()))
    out = out.cpu()
    assert torch.isfinite(out).all()
    assert torch.equal(out, j2f(tgt)(x, lens).cpu())                        # the class is this call
    for b, l in enumerate(lens):
        alone = j2f(tgt)(batch[b, :l].to(DEV)).cpu()
        assert alone.shape == (l - 1, 263) and torch.equal(out[b, :l - 1], alone), (b, l)
        assert (out[b, l - 1:] == 0).all()
        assert np.array_equal(out[b, :l - 1, 259:].numpy(), case(l, with_target)[2][:, 259:])


def test_normalised_output_is_the_raw_output_normalised():
    gen = torch.Generator().manual_seed(5)
    mean, std = torch.randn(263, generator=gen), 0.5 + 1.5 * torch.rand(263, generator=gen)
    lens = [197, 40, 3]
    batch = torch.zeros(3, 197, 22, 3)
    for b, l in enumerate(lens):
        batch[b, :l] = torch.from_numpy(case(l, False)[0]).float()
    op = Joints2Feats(mean, std)
    raw, got = op(batch.to(DEV), lens), op(batch.to(DEV), lens, normalize=True)
    want = (raw - mean.to(DEV)) / std.to(DEV)
    for b, l in enumerate(lens):
        g, w = got[b, :l - 1].cpu().numpy(), want[b, :l - 1].cpu().numpy()
        ulps = np.abs(g.astype(np.float64) - w) / np.spacing(np.abs(w)).astype(np.float64)
        print(f"normalised, {l} frames: max {ulps.max():.2f} ulp")
        assert ulps.max() <= 2                                               # the subtraction and the division each round once
        assert (got[b, l - 1:] == 0).all() and (raw[b, l - 1:] == 0).all()   # padding stays zero in both modes


def test_single_motion_and_input_forms():
    x = dev32(case(40, False)[0])
    op = j2f()
    one, batched = op(x), op(x[None], [40])
    assert one.shape == (39, 263) and batched.shape == (1, 39, 263) and torch.equal(one, batched[0])
    strided = torch.zeros(40, 22, 6, device=DEV)[..., ::2]                   # non-contiguous: accepted, copied
    strided.copy_(x)
    assert not strided.is_contiguous() and torch.equal(op(strided), one)
    assert torch.equal(op(x.double()).float(), one) and op(x.double()).dtype == torch.float64
    empty = op(torch.zeros(0, 40, 22, 3, device=DEV), [])
    assert empty.shape == (0, 39, 263) and empty.device == x.device
    pose = ref.target_pose()
    assert torch.equal(Joints2Feats(target_pose=pose)(x), j2f(ref.get_offsets_joints(pose))(x))
    assert not torch.equal(Joints2Feats(target_pose=pose)(x), one)
    assert not torch.equal(Joints2Feats(feet_thre=0.01)(x)[:, 259:], one[:, 259:])      # the threshold is the caller's


def test_edit_takes_joints_as_its_source():
    """`edit(batch["joints"])` is `edit(batch["motion"] = Joints2Feats(...)(joints, normalize=True))` bit for bit: 2 prompts, 40 source
    frames, 6 steps, fixed seeds and eps - as a padded tensor and as a list."""
    den = LADiffDenoiser(ABL, **DEN_KW); den.load_state_dict(syn.denoiser_weights(), strict=True)
    vae = LADiffVae(ABL, **VAE_KW); vae.load_state_dict(syn.vae_weights(263), strict=True)
    gen = torch.Generator().manual_seed(97)
    enc_out, eps = torch.randn(4, 1, 768, generator=gen), torch.randn(5, 2, 256, generator=gen).to(DEV)
    mean, std = 0.1 * torch.randn(263, generator=gen), 0.5 + torch.rand(263, generator=gen)
    dm = SimpleNamespace(feats2joints=None, hparams=SimpleNamespace(mean=mean.numpy(), std=std.numpy()), njoints=22)
    model = LADIFF(None, dm, denoiser=den.to(DEV).eval(), vae=vae.to(DEV).eval(), text_encoder=lambda texts: enc_out.to(DEV), guidance_scale=7.5,
                   num_inference_timesteps=6, eta=0.0, max_it=5,
                   scheduler=DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                           set_alpha_to_one=False, steps_offset=1, clip_sample=False))
    joints = torch.stack([torch.from_numpy(ref.motion(40, s)).float() for s in (1, 2)]).to(DEV)
    base = {"text": ["a", "b"], "length": [40, 60]}
    kw = dict(seeds=[11, 12], eps=eps)
    got = model.edit({**base, "joints": joints}, [0.5, 0.8], **kw)
    motion = Joints2Feats(mean, std)(joints, [40, 40], normalize=True)
    assert motion.shape == (2, 39, 263)
    want = model.edit({**base, "motion": motion, "source_length": [39, 39]}, [0.5, 0.8], **kw)
    as_list = model.edit({**base, "joints": [joints[0].cpu(), joints[1].cpu()]}, [0.5, 0.8], **kw)
    for b, l in enumerate(base["length"]):
        assert got[b].shape == (l, 22, 3) and torch.isfinite(got[b]).all()
        assert torch.equal(got[b], want[b]) and torch.equal(as_list[b], want[b])
    other = model.edit({**base, "joints": joints.flip(0)}, [0.5, 0.8], **kw)
    assert not torch.equal(other[0], got[0])                                 # the source matters
    # what `forward` returned goes back in: joints of a decoded motion are a valid source
    again = model.edit({**base, "joints": [g for g in got]}, 0.5, **kw)
    assert all(torch.isfinite(a).all() for a in again)
