"""Stage 1 (TRAIN.STAGE: vae) on the CPU: the fp64 restatements of tests/vae_stage_ref.py against the loss values the reference computed
for the goldens (tests/golden/make_golden_vae_stage.py), and the host-side plumbing - `LADIFF` reads the stage, `LADiffVae` the DVAE
keys, `MLDLosses` the lambdas.  Nothing here calls a kernel."""
import copy

import numpy as np
import pytest
import torch

from ladiff_amd import LADIFF, DDIMScheduler, LADiffDenoiser, LADiffVae, MLDLosses
from ladiff_amd.schema import ABL, DEN_KW, VAE_KW
from oracle import ladiff_oracle as orc
from conftest import load_golden
import vae_stage_ref as ref

SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False)
# The reference sums fp32 terms pairwise: about log2(n) 2^-24 = 1.4e-6 relative for n <= 1e7 positive terms; 1e-5 leaves room for the fp32
# rounding of each term and of the joints.
REF_RTOL = 1e-5


@pytest.mark.parametrize("name", ["vae_stage_humanml", "vae_stage_kit"])
def test_restatements_equal_the_reference_losses(name):
    g = load_golden(name)
    J = int(g["njoints"])
    joints_rst = orc.feats2joints(g["m_rst"], g["mean"], g["std_feats"], J)
    joints_ref = orc.feats2joints(g["features"], g["mean"], g["std_feats"], J)
    got = {"recons_feature": ref.smooth_l1(g["m_rst"], g["features"]), "recons_joints": ref.smooth_l1(joints_rst, joints_ref),
           "kl_motion": ref.kl_standard_normal(g["mu"], g["std"])}
    for key, value in got.items():
        want = float(g[key])
        print(f"{name} {key}: restated {value:.9g}, reference {want:.9g}, relative {abs(value - want) / abs(want):.2e}")
    for key, value in got.items():
        assert abs(value - float(g[key])) <= REF_RTOL * abs(float(g[key])), key
    # both SmoothL1 branches are exercised, and the golden's noise field is what (positions, values) restate
    d = (g["m_rst"] - g["features"]).abs()
    assert 0.1 < (d >= 1).float().mean().item() < 0.9
    assert g["positions"].unique().numel() == g["positions"].numel() and g["values"].shape == (g["features"].shape[0], g["positions"].numel())
    noisy = ref.corrupt(g["features"], g["positions"], g["values"])
    flat = noisy.reshape(noisy.shape[0], -1) - g["features"].numpy().reshape(noisy.shape[0], -1)
    untouched = np.ones(flat.shape[1], dtype=bool)
    untouched[g["positions"].numpy()] = False
    assert not flat[:, untouched].any() and np.abs(flat[:, ~untouched]).min() > 0


def test_smooth_l1_restatement_at_the_branch_point():
    d = np.array([0.0, 0.5, np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0), -1.0, -3.0])
    want = np.array([0.0, 0.125, 0.5 * np.nextafter(1.0, 0.0) ** 2, 0.5, np.nextafter(1.0, 2.0) - 0.5, 0.5, 2.5])
    for x, w in zip(d, want):
        assert ref.smooth_l1(np.array([x]), np.array([0.0])) == w
    assert ref.kl_standard_normal(np.zeros(3), np.ones(3)) == 0.0


def _model(**kw):
    den, vae = LADiffDenoiser(ABL, **DEN_KW), LADiffVae(ABL, **VAE_KW)
    return LADIFF(kw.pop("cfg", None), None, denoiser=den, vae=vae, scheduler=DDIMScheduler(set_alpha_to_one=False, steps_offset=1, **SCHED_KW),
                  text_encoder=lambda t: None, **kw)


def test_ladiff_reads_the_stage():
    assert _model().stage == "diffusion"
    cfg = {"TRAIN": {"STAGE": "vae"}, "model": {"condition": "text_uncond", "vae": False}}
    m = _model(cfg=cfg)
    assert m.stage == "vae" and m.condition == "text_uncond" and m.is_vae is False
    assert _model(cfg=cfg, stage="diffusion").stage == "diffusion"            # the keyword wins
    d = _model(stage="vae")
    assert d.stage == "vae" and d.condition == "text" and d.is_vae is True
    with pytest.raises(NotImplementedError):
        _model(stage="vae_diffusion")
    with pytest.raises(NotImplementedError):
        _model(cfg={"TRAIN": {"STAGE": "vae_diffusion"}})
    with pytest.raises(ValueError):
        _model(stage="stage1")


def test_vae_exposes_the_dvae_keys():
    v = LADiffVae(ABL, **VAE_KW)
    assert v.dvae is False and v.percentage_noised == 0.0
    abl = copy.copy(ABL)
    abl.DVAE, abl.PERCENTAGE_NOISED = True, 0.33
    v = LADiffVae(abl, **VAE_KW)
    assert v.dvae is True and v.percentage_noised == 0.33
    # the default draw: the reference's np.random.choice call on the global stream, its distinct values, one normal each
    np.random.seed(3)
    positions, values = v.draw_corruption(2, 7, "cpu")
    np.random.seed(3)
    want = np.unique(np.random.choice(7 * 263, int(7 * 263 * 0.33)))
    assert positions.dtype == torch.int64 and positions.tolist() == want.tolist() and values.shape == (2, len(want))
    with pytest.raises(ValueError):
        v._corruption_table((torch.tensor([1, 1]), torch.zeros(2, 2)), 2, 7, "cpu")          # not distinct
    with pytest.raises(ValueError):
        v._corruption_table((torch.tensor([7 * 263]), torch.zeros(2, 1)), 2, 7, "cpu")       # outside [F, C]
    with pytest.raises(ValueError):
        v._corruption_table((torch.tensor([0, 5]), torch.zeros(3, 2)), 2, 7, "cpu")          # values of another batch
    slot, vals, n = v._corruption_table((torch.tensor([5, 0]), torch.ones(2, 2)), 2, 7, "cpu")
    assert n == 2 and slot.dtype == torch.int32 and slot[5] == 0 and slot[0] == 1 and int((slot >= 0).sum()) == 2


def test_losses_take_their_lambdas_from_the_config():
    d = MLDLosses()
    assert d.stage == "vae" and d._params["recons_feature"] == 1.0 and d._params["recons_joints"] == 1.0 and d._params["kl_motion"] == 1e-4
    cfg = {"TRAIN": {"STAGE": "vae"}, "LOSS": {"LAMBDA_REC": 2.0, "LAMBDA_JOINT": 0.25, "LAMBDA_KL": 1e-3, "LAMBDA_GEN": 3.0}}
    m = MLDLosses(True, "xyz", cfg)
    assert m._params["recons_feature"] == 2.0 and m._params["kl_motion"] == 1e-3
    assert m._params["recons_joints"] == 0.25 and m._params["gen_joints"] == 0.25          # a key ending in `joints`: LAMBDA_JOINT
    assert m._params["gen_feature"] == 3.0
    k = MLDLosses(lambda_rec=0.5, lambda_joint=4.0, lambda_kl=0.0)
    assert (k._params["recons_feature"], k._params["recons_joints"], k._params["kl_motion"]) == (0.5, 4.0, 0.0)
    assert m.losses == ["recons_feature", "recons_verts", "recons_joints", "recons_limb", "gen_feature", "gen_joints", "kl_motion", "total"]
    assert m.loss2logname("total", "val") == "total/val" and m.loss2logname("recons_feature", "val") == "recons/feature/val"
    assert m.count == 0 and set(m.compute()) == set(m.losses)
    for stage in ("diffusion", "vae_diffusion"):
        with pytest.raises(NotImplementedError):
            MLDLosses(stage=stage)
    with pytest.raises(NotImplementedError):
        MLDLosses(cfg={"TRAIN": {"STAGE": "diffusion"}})
    with pytest.raises(ValueError):
        MLDLosses(stage="other")
    m.add_sums({"count": 2, "sums": [2.0, 4.0, 6.0, 8.0]})
    out = m.compute()
    assert (out["recons_feature"], out["recons_joints"], out["kl_motion"], out["total"], out["gen_joints"]) == (1.0, 2.0, 3.0, 4.0, 0.0)
    if not torch.cuda.is_available():
        from ladiff_amd import _lib
        z = torch.zeros(1, 2, 263)
        n = torch.distributions.Normal(torch.zeros(1, 1, 256), torch.ones(1, 1, 256))
        with pytest.raises(_lib.LadiffHipError):                    # no CPU path
            m.update({"m_rst": z, "m_ref": z, "joints_rst": torch.zeros(1, 2, 22, 3), "joints_ref": torch.zeros(1, 2, 22, 3), "dist_m": n,
                      "dist_ref": torch.distributions.Normal(torch.zeros(1, 1, 256), torch.ones(1, 1, 256))})
