"""Stage 1 (TRAIN.STAGE: vae) on the GPU: the DVAE input corruption of `LADiffVae.encode` against goldens captured from the reference
(tests/golden/make_golden_vae_stage.py), the stage-"vae" losses (`ladiff_vae_losses` through `MLDLosses`) against the fp64 restatements of
tests/vae_stage_ref.py, the VAE branches of `LADIFF.t2m_eval` / `train_vae_forward` / `mm_eval` against the same pieces composed by hand
under the same seeds, and the two new entries held to the memory contract.  Synthetic weights; stub datamodule, text encoder and
evaluators as in test_gpu_mm_eval.py."""
import copy
import ctypes
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ladiff_amd import (LADIFF, DDIMScheduler, LADiffDenoiser, LADiffVae, MLDLosses, MotionEncoderBiGRUCo, MovementConvEncoder,
                        TextEncoderBiGRUCo, _lib, synthetic as syn, validate)
from ladiff_amd.schema import ABL, DEN_KW, VAE_KW
from oracle import ladiff_oracle as orc
from conftest import load_golden
from memory_contract import FILLS, Out, assert_contract, assert_refused, run_fills, run_in_guards
import vae_stage_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False)
FRAME_TOL = 1e-3                  # the project's one gate: max |decoded frame - reference frame|
SUM_RTOL = 1e-9                   # fp64 sums of n <= 1e7 terms in another order: n 2^-53 = 1e-9 at most, plus one-ulp `log` differences
REF_RTOL = 1e-5                   # against the reference's fp32 pairwise sums (tests/test_vae_stage.py)
DVAE_ABL = copy.copy(ABL)
DVAE_ABL.DVAE, DVAE_ABL.PERCENTAGE_NOISED = True, 0.33


def maxdiff(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


def make_vae(nfeats, abl=ABL):
    m = LADiffVae(abl, **{**VAE_KW, "nfeats": nfeats})
    m.load_state_dict(syn.vae_weights(nfeats), strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def vaes():
    return {(C, dvae): make_vae(C, DVAE_ABL if dvae else ABL) for C in (263, 251) for dvae in (False, True)}


def raw_encode(vae, feats, lens, eps):
    """`ladiff_vae_encode`, the entry as it was before this stage existed, called directly."""
    L = _lib.lib()
    B, F, C = feats.shape
    T = vae.max_it
    wt = vae._weight_table("encoder")
    out = [torch.empty(T, B, 256, device=DEV) for _ in range(3)]
    wsb = L.ladiff_encoder_workspace_bytes(B, F, T, C)
    ws = _lib.workspace(wsb, DEV)
    ints = lambda v: torch.tensor(list(v), dtype=torch.int32, device=DEV)
    ld, cd = ints(lens), ints(syn.max_iter_elements(lens))
    _lib.check(L.ladiff_vae_encode(wt.array, wt.split_array() if _lib.is_split(vae.precision) else None, _lib.ptr(feats), ld.data_ptr(),
                                   cd.data_ptr(), _lib.ptr(eps), B, F, T, C, *(_lib.ptr(o) for o in out), _lib.ptr(ws), wsb, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------- DVAE encode
@pytest.mark.parametrize("name,nfeats,precision", [("vae_stage_humanml", 263, "fp32"), ("vae_stage_kit", 251, "fp32"),
                                                   ("vae_stage_humanml", 263, "f16x3")])
def test_dvae_encode_golden(vaes, name, nfeats, precision):
    """The reference's encode with DVAE=True on the recorded noise field; gates of test_gpu_path.py::test_vae_encode_golden."""
    g = load_golden(name)
    v = vaes[(nfeats, True)]
    v.precision = precision
    try:
        lens = g["lengths"].tolist()
        feats, eps = g["features"].to(DEV), g["eps"].to(DEV)
        latent, dist, counts = v.encode(feats, lens, eps=eps, corrupt=(g["positions"], g["values"].to(DEV)))
        assert counts.tolist() == g["counts"].tolist() and latent.shape == g["latent"].shape
        tol = 1e-4 if precision == "fp32" else 2e-3
        e_mu, e_std, e_lat = maxdiff(dist.loc, g["mu"]), maxdiff(dist.scale, g["std"]), maxdiff(latent, g["latent"])
        print(f"DVAE encode {name} {precision}: mu {e_mu:.3e} std {e_std:.3e} (max {g['std'].max().item():.2f}) latent {e_lat:.3e}")
        assert e_mu < tol and e_std < tol * max(1.0, g["std"].max().item())
        assert e_lat < tol * max(1.0, g["latent"].abs().max().item())
        for i, c in enumerate(g["counts"].tolist()):
            assert c == latent.shape[0] or latent[c:, i].abs().max().item() == 0
        # the corruption matters at this tolerance: the clean input lands elsewhere
        clean, cdist, _ = v.encode(feats, lens, eps=eps, corrupt=(torch.zeros(0, dtype=torch.long), torch.zeros(len(lens), 0)))
        assert maxdiff(cdist.loc, g["mu"]) > 10 * tol
        # ... and with the noise cleared the new entry gives today's encode bit for bit
        mu0, std0, lat0 = raw_encode(v, feats, lens, eps)
        assert torch.equal(cdist.loc, mu0) and torch.equal(cdist.scale, std0) and torch.equal(clean, lat0)
    finally:
        v.precision = "fp32"


def test_dvae_default_draw_and_dvae_off(vaes):
    """DVAE=True, nothing given: the positions come from the global numpy stream through the reference's own call and the values from
    torch's generator, before the rsample draw - the same bits as `corrupt=` built by hand from the two seeds.  DVAE=False: today's
    entry, bit for bit."""
    g = load_golden("vae_stage_kit")
    feats, lens = g["features"].to(DEV), g["lengths"].tolist()
    B, F, C = feats.shape
    v = vaes[(251, True)]
    np.random.seed(11); torch.manual_seed(12)
    lat, dist, _ = v.encode(feats, lens)
    np.random.seed(11); torch.manual_seed(12)
    positions = torch.from_numpy(np.unique(np.random.choice(F * C, int(F * C * 0.33))))
    values = torch.randn(B, positions.numel(), device=DEV)
    eps = torch.randn(5, B, 256, device=DEV)
    lat2, dist2, _ = v.encode(feats, lens, eps=eps, corrupt=(positions, values))
    assert torch.equal(lat, lat2) and torch.equal(dist.loc, dist2.loc) and torch.equal(dist.scale, dist2.scale)
    assert 0.25 * F * C < positions.numel() < 0.33 * F * C
    off = vaes[(251, False)]
    assert off.dvae is False
    lat3, dist3, _ = off.encode(feats, lens, eps=eps)
    mu0, std0, lat0 = raw_encode(off, feats, lens, eps)
    assert torch.equal(lat3, lat0) and torch.equal(dist3.loc, mu0) and torch.equal(dist3.scale, std0)
    assert maxdiff(dist3.loc, dist.loc) > 1e-3                      # the corrupted encode is another result
    # an explicit corrupt is honoured without DVAE too
    lat4, dist4, _ = off.encode(feats, lens, eps=eps, corrupt=(positions, values))
    assert torch.equal(lat4, lat2) and torch.equal(dist4.loc, dist2.loc)


@pytest.mark.parametrize("name,nfeats,precision", [("vae_stage_humanml", 263, "fp32"), ("vae_stage_kit", 251, "fp32"),
                                                   ("vae_stage_humanml", 263, "f16x3")])
def test_decode_of_the_golden_latent(vaes, name, nfeats, precision):
    """decode(golden latent) against the reference's reconstruction within the frame gate; the encode -> decode chain error is
    measured and printed (nobody has measured it before: not gated)."""
    g = load_golden(name)
    v = vaes[(nfeats, True)]
    v.precision = precision
    try:
        lens = g["lengths"].tolist()
        rst = v.decode(g["latent"].to(DEV), lens)
        err = maxdiff(rst, g["m_rst"])
        lat, _, _ = v.encode(g["features"].to(DEV), lens, eps=g["eps"].to(DEV), corrupt=(g["positions"], g["values"].to(DEV)))
        chain = maxdiff(v.decode(lat, lens), g["m_rst"])
        print(f"stage-1 chain {name} {precision}: decode(golden latent) {err:.3e}, encode -> decode {chain:.3e} (max |m_rst| "
              f"{g['m_rst'].abs().max().item():.2f})")
        assert rst.shape == g["m_rst"].shape and err < FRAME_TOL
    finally:
        v.precision = "fp32"


# ---------------------------------------------------------------- losses
def loss_inputs(B, F, C, J, T, seed=0, misalign=False):
    gen = torch.Generator().manual_seed(seed + B * F + C + T)

    def place(t):                                                   # misalign: the tensor starts 4 bytes past a 16-byte boundary
        if not misalign:
            return t.to(DEV)
        buf = torch.empty(t.numel() + 1, device=DEV)
        buf[1:] = t.reshape(-1).to(DEV)
        out = buf[1:].view(t.shape)
        assert out.data_ptr() % 16 == 4 and out.is_contiguous()
        return out
    shapes = [(B, F, C), (B, F, C), (B, F, J, 3), (B, F, J, 3), (T, B, 256)]
    m_rst, m_ref, j_rst, j_ref, mu = (place(torch.randn(*s, generator=gen)) for s in shapes)
    std = place(torch.exp(torch.empty(T, B, 256).uniform_(float(np.log(0.17)), float(np.log(6.4)), generator=gen)))
    return m_rst, m_ref, j_rst, j_ref, mu, std


def rs_of(m_rst, m_ref, j_rst, j_ref, mu, std):
    return {"m_rst": m_rst, "m_ref": m_ref, "joints_rst": j_rst, "joints_ref": j_ref, "dist_m": torch.distributions.Normal(mu, std),
            "dist_ref": torch.distributions.Normal(torch.zeros_like(mu), torch.ones_like(std))}


def rel(got, want):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / np.abs(np.asarray(want))))


@pytest.mark.parametrize("shape", [(1, 1, 263, 22, 1), (3, 60, 263, 22, 5), (2, 33, 251, 21, 5), (16, 196, 263, 22, 5)])
def test_losses_equal_the_fp64_restatement(shape):
    """Fewer elements than one wave | the HumanML golden shape | element counts that are no multiple of 4 | many workgroups of partials."""
    lam = dict(lambda_rec=1.0, lambda_joint=0.5, lambda_kl=1e-4)
    a = loss_inputs(*shape)
    want = ref.losses(*a, **lam)
    m = MLDLosses(**lam)
    total = m.update(rs_of(*a))
    assert total.dim() == 0 and total.is_cuda and total.dtype == torch.float64
    got = m.last_batch.cpu().numpy()
    print(f"losses {shape}: device {got.tolist()} relative to the restatement {rel(got, want):.2e}")
    assert rel(got, want) < SUM_RTOL and total.item() == got[3]
    # the same elements from addresses that are not 16-byte aligned (the scalar loads): the same bits
    m2 = MLDLosses(**lam)
    m2.update(rs_of(*loss_inputs(*shape, misalign=True)))
    assert np.array_equal(m2.last_batch.cpu().numpy(), got)
    # two updates: identical bits, the accumulator holds exactly their sum, compute() divides by the count
    m.update(rs_of(*a))
    assert np.array_equal(m.last_batch.cpu().numpy(), got)
    st = m.sums()
    assert st["count"] == 2 and np.array_equal(st["sums"], got + got)
    out = m.compute()
    assert [out[k] for k in ("recons_feature", "recons_joints", "kl_motion", "total")] == ((got + got) / 2.0).tolist()
    assert out["recons_verts"] == 0.0 and out["gen_joints"] == 0.0 and set(out) == set(m.losses)
    m.reset()
    assert m.count == 0 and not m.sums()["sums"].any()


def test_losses_at_the_smooth_l1_branch_point():
    """Every |d| exactly below, at and above 1 (both signs), against the restatement; and sigma = 1, mu = 0 gives a KL of exactly 0."""
    one = np.float32(1.0)
    edge = np.array([np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(2))], dtype=np.float32)
    B, F, C, J, T = 1, 3, 263, 22, 1
    for k, d in enumerate(edge):
        sign = torch.where(torch.arange(B * F * C) % 2 == 0, 1.0, -1.0).reshape(B, F, C)
        m_ref = torch.zeros(B, F, C)
        m_rst = m_ref + sign * float(d)
        j_ref = torch.zeros(B, F, J, 3)
        j_rst = j_ref - float(d)
        mu, std = torch.zeros(T, B, 256), torch.ones(T, B, 256)
        a = [t.to(DEV) for t in (m_rst, m_ref, j_rst, j_ref, mu, std)]
        m = MLDLosses()
        m.update(rs_of(*a))
        got, want = m.last_batch.cpu().numpy(), ref.losses(*a)
        term = 0.5 * float(d) ** 2 if d < 1 else float(d) - 0.5
        print(f"|d| = {float(d)!r}: device {got[:2].tolist()}, one term {term!r}")
        assert abs(got[0] - term) <= SUM_RTOL * term and abs(got[1] - term) <= SUM_RTOL * term and got[2] == 0.0
        assert rel(got[[0, 1, 3]], want[[0, 1, 3]]) < SUM_RTOL


@pytest.mark.parametrize("name", ["vae_stage_humanml", "vae_stage_kit"])
def test_losses_equal_the_reference_values(name):
    g = load_golden(name)
    J = int(g["njoints"])
    j_rst = orc.feats2joints(g["m_rst"], g["mean"], g["std_feats"], J)
    j_ref = orc.feats2joints(g["features"], g["mean"], g["std_feats"], J)
    a = [t.to(DEV) for t in (g["m_rst"], g["features"], j_rst, j_ref, g["mu"], g["std"])]
    m = MLDLosses()
    m.update(rs_of(*a))
    out = m.compute()
    for key in ("recons_feature", "recons_joints", "kl_motion"):
        want = float(g[key])
        print(f"{name} {key}: device {out[key]:.9g}, reference {want:.9g}, relative {abs(out[key] - want) / abs(want):.2e}")
    for key in ("recons_feature", "recons_joints", "kl_motion"):
        assert abs(out[key] - float(g[key])) <= REF_RTOL * abs(float(g[key])), key
    assert rel(m.last_batch.cpu().numpy(), ref.losses(*a)) < SUM_RTOL


def test_losses_refuse_what_is_not_built():
    a = loss_inputs(1, 2, 263, 22, 1)
    rs = rs_of(*a)
    m = MLDLosses()
    with pytest.raises(NotImplementedError):                        # model.vae: false hands dist_m itself as dist_ref
        m.update({**rs, "dist_ref": rs["dist_m"]})
    with pytest.raises(NotImplementedError):
        m.update({**rs, "dist_ref": torch.distributions.Normal(torch.zeros_like(a[4]), 2 * torch.ones_like(a[5]))})
    with pytest.raises(_lib.LadiffHipError):
        m.update({**rs, "joints_rst": a[2][:, :1]})
    assert m.count == 0


# ---------------------------------------------------------------- LADIFF in stage "vae"
class StubText:
    def __init__(self):
        self.calls = []

    def __call__(self, texts):
        self.calls.append(list(texts))
        rows = [torch.randn(768, generator=torch.Generator().manual_seed(zlib.crc32(t.encode()))) for t in texts]
        return torch.stack(rows).unsqueeze(1).to(DEV)


@pytest.fixture(scope="module")
def nets(vaes):
    den = LADiffDenoiser(ABL, **DEN_KW); den.load_state_dict(syn.denoiser_weights(), strict=True)
    mv, mo, tx = syn.t2m_weights(263)
    move = MovementConvEncoder(259, 512, 512); move.load_state_dict(mv, strict=True)
    motion = MotionEncoderBiGRUCo(512, 1024, 512); motion.load_state_dict(mo, strict=True)
    text = TextEncoderBiGRUCo(300, 15, 512, 512); text.load_state_dict(tx, strict=True)
    return den.to(DEV).eval(), vaes, (text.to(DEV), move.to(DEV), motion.to(DEV))


def datamodule(identity_renorm=False):
    rs = np.random.RandomState(2)
    mean = torch.from_numpy(rs.standard_normal(263).astype(np.float32)) * 0.1
    std = torch.from_numpy(rs.uniform(0.5, 1.5, 263).astype(np.float32))
    mean_e = torch.from_numpy(rs.standard_normal(263).astype(np.float32)) * 0.1
    std_e = torch.from_numpy(rs.uniform(0.5, 1.5, 263).astype(np.float32))

    def renorm(f):
        d = f.device
        return (f * std.to(d) + mean.to(d) - mean_e.to(d)) / std_e.to(d)

    return SimpleNamespace(renorm4t2m=(lambda f: f) if identity_renorm else renorm, mean=mean, std=std, njoints=22, is_mm=False,
                           feats2joints=lambda f: orc.feats2joints(f, mean, std, 22))


def make_model(nets, dvae=True, cfg=None, dm=None, **kw):
    den, vaes, evaluators = nets
    stub = StubText()
    model = LADIFF(cfg, dm if dm is not None else datamodule(), denoiser=den, vae=vaes[(263, dvae)],
                   scheduler=DDIMScheduler(set_alpha_to_one=False, steps_offset=1, **SCHED_KW), guidance_scale=7.5,
                   num_inference_timesteps=5, eta=0.0, text_encoder=stub, **kw)
    model.set_t2m_evaluators(*evaluators, unit_len=4)
    return model, stub


def make_batch(lens, seed=63):
    gen = torch.Generator().manual_seed(seed)
    B = len(lens)
    motions = torch.randn(B, max(lens), 263, generator=gen)
    for i, l in enumerate(lens):
        motions[i, l:] = 0
    cap = torch.tensor(sorted(torch.randint(2, 13, (B,), generator=gen).tolist(), reverse=True))
    word = torch.randn(B, 12, 300, generator=gen)
    pos = torch.nn.functional.one_hot(torch.randint(0, 15, (B, 12), generator=gen), 15).float()
    return {"text": [f"motion number {i}" for i in range(B)], "length": list(lens), "motion": motions, "word_embs": word, "pos_ohot": pos,
            "text_len": cap}


def seed_all(s):
    np.random.seed(s)
    torch.manual_seed(s + 1)


def test_t2m_eval_in_stage_vae(nets):
    """3 motions, F = 60: every entry of rs_set is the by-hand composition encode -> decode -> feats2joints -> renorm -> sort ->
    evaluators, bit for bit under the same seeds; no text encoder call, no loop plan."""
    lens = [24, 60, 49]
    batch = make_batch(lens)
    model, stub = make_model(nets, stage="vae")
    seed_all(5)
    rs = model.t2m_eval(batch)
    assert stub.calls == [] and model._plans == {}
    seed_all(5)
    vae, dm = model.vae, model.datamodule
    motions = batch["motion"].to(DEV)
    z, _, _ = vae.encode(motions, lens)
    feats = vae.decode(z, lens)
    joints_rst, joints_ref = model.feats2joints_device(feats), model.feats2joints_device(motions)
    idx = torch.as_tensor(np.argsort(lens)[::-1].copy(), device=DEV)
    feats_s, motions_s = dm.renorm4t2m(feats)[idx], dm.renorm4t2m(motions)[idx]
    m_lens = torch.tensor(lens, device=DEV)[idx] // 4
    want = {"m_ref": motions_s, "m_rst": feats_s,
            "lat_t": model.t2m_textencoder(batch["word_embs"].to(DEV), batch["pos_ohot"].to(DEV), batch["text_len"])[idx],
            "lat_m": model.t2m_motionencoder(model.t2m_moveencoder(motions_s[..., :-4]), m_lens),
            "lat_rm": model.t2m_motionencoder(model.t2m_moveencoder(feats_s[..., :-4]), m_lens),
            "joints_ref": joints_ref, "joints_rst": joints_rst}
    assert set(rs) == set(want)
    for key in want:
        print(f"stage-1 t2m_eval vs by hand: {key} {tuple(want[key].shape)} max abs diff {maxdiff(rs[key], want[key]):.3e}")
    for key in want:
        assert rs[key].shape == want[key].shape and torch.equal(rs[key], want[key]), key
    assert rs["m_rst"].shape == (3, 60, 263) and torch.isfinite(rs["m_rst"]).all()
    # condition text_uncond: the latents are replaced by a standard-normal draw
    uncond, ustub = make_model(nets, cfg={"TRAIN": {"STAGE": "vae"}, "model": {"condition": "text_uncond"}})
    assert uncond.stage == "vae" and uncond.condition == "text_uncond"
    seed_all(5)
    ru = uncond.t2m_eval(batch)
    assert ustub.calls == [] and uncond._plans == {}
    assert maxdiff(ru["m_rst"], rs["m_rst"]) > FRAME_TOL and torch.equal(ru["m_ref"], rs["m_ref"])
    # the default stage on the same batch still runs the loop
    default, dstub = make_model(nets)
    assert default.stage == "diffusion"
    seed_all(5)
    rd = default.t2m_eval(batch)
    assert len(dstub.calls) == 1 and len(default._plans) >= 1 and default.loop_status() == (0, 0)
    assert rd["m_rst"].shape == rs["m_rst"].shape and maxdiff(rd["m_rst"], rs["m_rst"]) > FRAME_TOL


def test_forward_in_stage_vae(nets):
    lens = [24, 60]
    batch = make_batch(lens)
    model, stub = make_model(nets, stage="vae")
    seed_all(7)
    joints = model(batch)
    assert stub.calls == [] and model._plans == {}
    seed_all(7)
    z, _, _ = model.vae.encode(batch["motion"].to(DEV), lens)
    want = model.feats2joints_device(model.vae.decode(z, lens)).cpu()
    assert [tuple(j.shape) for j in joints] == [(24, 22, 3), (60, 22, 3)]
    assert all(torch.equal(j, want[i, :l]) for i, (j, l) in enumerate(zip(joints, lens)))


def test_train_vae_forward_and_validate(nets):
    lens = [24, 60, 49]
    b1, b2 = make_batch(lens, seed=1), make_batch([33, 7], seed=2)
    model, stub = make_model(nets, stage="vae")
    seed_all(9)
    rs = model.train_vae_forward(b1)
    assert set(rs) == {"m_ref", "m_rst", "lat_m", "lat_rm", "joints_ref", "joints_rst", "dist_m", "dist_ref"}
    assert rs["m_ref"].shape == rs["m_rst"].shape == (3, 60, 263) and rs["lat_m"].shape == rs["lat_rm"].shape == (3, 5, 256)
    assert rs["joints_ref"].shape == rs["joints_rst"].shape == (3, 60, 22, 3)
    assert rs["dist_m"].loc.shape == rs["dist_m"].scale.shape == (5, 3, 256)
    assert not rs["dist_ref"].loc.any() and bool((rs["dist_ref"].scale == 1).all()) and rs["dist_ref"].loc.shape == (5, 3, 256)
    assert stub.calls == [] and model._plans == {}
    seed_all(9)
    vae = model.vae
    z, dist, _ = vae.encode(b1["motion"].to(DEV), lens)
    m_rst = vae.decode(z, lens)
    z2, _, _ = vae.encode(m_rst, lens)
    assert torch.equal(rs["lat_m"], z.permute(1, 0, 2)) and torch.equal(rs["m_rst"], m_rst) and torch.equal(rs["lat_rm"], z2.permute(1, 0, 2))
    assert torch.equal(rs["dist_m"].loc, dist.loc) and torch.equal(rs["dist_m"].scale, dist.scale)
    # model.vae: false hands dist_m back as dist_ref, which the losses refuse
    plain, _ = make_model(nets, cfg={"TRAIN": {"STAGE": "vae"}, "model": {"vae": False}})
    rp = plain.train_vae_forward(b2)
    assert rp["dist_ref"] is rp["dist_m"]
    # validate() over two batches = two manual updates
    lam = dict(lambda_rec=1.0, lambda_joint=1.0, lambda_kl=1e-4)
    seed_all(10)
    la = MLDLosses(**lam)
    out = validate(model, [b1, b2], losses=la)
    seed_all(10)
    lb = MLDLosses(**lam)
    t1 = lb.update(model.train_vae_forward(b1))
    t2 = lb.update(model.train_vae_forward(b2))
    assert la.count == 2 and np.array_equal(la.sums()["sums"], lb.sums()["sums"]) and out == lb.compute()
    assert out["total"] == (t1.item() + t2.item()) / 2.0 and all(np.isfinite(v) for v in out.values())
    want = ref.losses(rs["m_rst"], rs["m_ref"], rs["joints_rst"], rs["joints_ref"], rs["dist_m"].loc, rs["dist_m"].scale, **lam)
    solo = MLDLosses(**lam)
    solo.update(rs)
    assert rel(solo.last_batch.cpu().numpy(), want) < SUM_RTOL
    print("validate():", {k: round(v, 6) for k, v in out.items()})
    seed_all(10)
    assert validate(model, [b1, b2])["total"] == out["total"]        # default-constructed losses: the same lambdas


def test_mm_eval_in_stage_vae(nets):
    """2 motions x R = 4 with encode / decode calls of at most 3 rows (cut mid-prompt) against the uncut call under the same seeds."""
    lens, R = [60, 24], 4
    batch = make_batch(lens, seed=4)
    out, lat = {}, {}
    for cap in (320, 3):
        model, stub = make_model(nets, stage="vae", dm=datamodule(identity_renorm=True), max_prompts_per_launch=cap)
        seed_all(21)
        out[cap] = model.mm_eval(batch, repeats=R)
        assert stub.calls == [] and model._plans == {}
        assert model.last_mm_launches == ([(0, 8)] if cap == 320 else [(0, 3), (3, 6), (6, 8)])
        seed_all(21)
        rows = batch["motion"].to(DEV).repeat_interleave(R, dim=0)
        lat[cap], _ = model._stage1_reconstruct(rows, [l for l in lens for _ in range(R)], model._row_cuts(8))
    rs = out[3]
    assert rs["lat_rm"].shape == (2, R, 512) and rs["m_rst"].shape == (8, 60, 263) and rs["joints_rst"].shape == (8, 60, 22, 3)
    assert rs["lengths"] == [60] * R + [24] * R
    d_z = maxdiff(lat[3], lat[320])
    d_lat, d_frames = maxdiff(out[3]["lat_rm"], out[320]["lat_rm"]), maxdiff(out[3]["m_rst"], out[320]["m_rst"])
    print(f"stage-1 mm_eval, 3 rows per call vs uncut: z {d_z:.3e}, lat_rm {d_lat:.3e}, frames {d_frames:.3e}")
    assert d_z < 1e-4 * max(1.0, lat[320].abs().max().item())     # the latent gate of test_vae_encode_decode_round_trip_full_size
    assert d_lat < FRAME_TOL and d_frames < FRAME_TOL              # as test_mm_eval_does_not_depend_on_the_packing holds another packing
    # prompt order: rows 4 .. 7 are the 24-frame motion (zero behind its length), and the R repeats are samples, not copies
    assert not rs["m_rst"][R:, 24:].any() and rs["m_rst"][:R, 24:].any()
    assert maxdiff(rs["m_rst"][0], rs["m_rst"][1]) > FRAME_TOL and maxdiff(rs["lat_rm"][1, 0], rs["lat_rm"][1, 3]) > 0
    # the MM branch of t2m_eval: the same rows through the same cut
    model, stub = make_model(nets, stage="vae", dm=datamodule(identity_renorm=True), mm_num_repeats=R)
    model.datamodule.is_mm = True
    seed_all(21)
    one = make_batch([60], seed=4)
    mm = model.t2m_eval(one)
    assert stub.calls == [] and mm["m_rst"].shape == (R, 60, 263) and mm["lat_rm"].shape == (R, 512)
    assert maxdiff(mm["m_rst"][0], mm["m_rst"][1]) > FRAME_TOL
    with pytest.raises(ValueError):
        model.mm_eval(batch, repeats=R, noise_seed=1)


# ---------------------------------------------------------------- memory contract of the two new entries
def hold(what, call, ws_bytes, outs, want, tol):
    assert_refused(run_in_guards(call, ws_bytes - 4, outs, FILLS["nan"]), what + ", workspace 4 bytes short")
    res = run_fills(call, ws_bytes, outs)
    rep = assert_contract(res, want, tol, what)
    print(f"memory contract | {what}: guard words touched {rep['guards']}, fills bit-identical: {rep['identical']}, "
          f"deterministic: {rep['deterministic']}")
    assert rep["identical"] and rep["deterministic"] and rep["guards"] == 0
    return res


@pytest.mark.parametrize("case,precision", [("smallest", "fp32"), ("vae_stage_humanml", "fp32"), ("vae_stage_humanml", "f16x3")])
def test_memory_contract_of_the_dvae_encode(vaes, case, precision):
    """B = F = 1 (two corrupted positions) against the CPU oracle on the corrupted input, and the HumanML golden; tolerances of
    test_gpu_path.py::test_vae_encode_golden."""
    T, C = 5, 263
    if case == "smallest":
        gen = torch.Generator().manual_seed(1)
        feats, eps, lens = torch.randn(1, 1, C, generator=gen), torch.randn(T, 1, 256, generator=gen), [1]
        positions, values = torch.tensor([0, 200]), torch.randn(1, 2, generator=gen)
        with torch.no_grad():
            mu, sd, lat = orc.vae_encode(syn.vae_weights(C), torch.from_numpy(ref.corrupt(feats, positions, values)), lens, eps)
    else:
        g = load_golden(case)
        feats, eps, lens, positions, values = g["features"], g["eps"], g["lengths"].tolist(), g["positions"], g["values"]
        mu, sd, lat = g["mu"], g["std"], g["latent"]
    B, F, _ = feats.shape
    v = vaes[(C, False)]
    wt = v._weight_table("encoder")
    wsplit = wt.split_array() if precision != "fp32" else None
    slot, vals, n = v._corruption_table((positions, values), B, F, DEV)
    ints = lambda x: torch.tensor(list(x), dtype=torch.int32, device=DEV)
    fd, ed, ld, cd = feats.to(DEV).contiguous(), eps.to(DEV).contiguous(), ints(lens), ints(syn.max_iter_elements(lens))
    L = _lib.lib()

    def call(ws, nb, o):
        return L.ladiff_vae_encode_dvae(wt.array, wsplit, _lib.ptr(fd), ld.data_ptr(), cd.data_ptr(), _lib.ptr(ed), B, F, T, C, o["mu"],
                                        o["std"], o["latent"], ws, nb, slot.data_ptr(), _lib.ptr(vals), n, _lib.stream_ptr())
    tol = 1e-4 if precision == "fp32" else 2e-3
    hold(f"ladiff_vae_encode_dvae {case} {precision}", call, L.ladiff_encoder_workspace_bytes(B, F, T, C),
         {k: Out(T * B, 256) for k in ("mu", "std", "latent")}, {"mu": mu, "std": sd, "latent": lat},
         {"mu": tol, "std": tol * max(1.0, sd.max().item()), "latent": tol * max(1.0, lat.abs().max().item())})


@pytest.mark.parametrize("shape", [(1, 1, 263, 22, 1), (3, 60, 263, 22, 5)])
def test_memory_contract_of_the_losses(shape):
    """`batch` and the workspace in guards under the three fills; `acc` is the one buffer the entry reads before it writes, by design: it
    is pre-set, sits between guard words of its own, and must have gained exactly `batch`."""
    B, F, C, J, T = shape
    a = loss_inputs(*shape, seed=3)
    want = ref.losses(*a, lambda_rec=1.0, lambda_joint=0.5, lambda_kl=1e-4)
    L = _lib.lib()
    preset = torch.tensor([1.5, -2.0, 1.0e6, 0.1], dtype=torch.float64)
    state = {}

    def call(ws, nb, o):
        buf = torch.full((68,), -7.25, dtype=torch.float64, device=DEV)
        buf[32:36] = preset.to(DEV)
        state["acc"] = buf
        return L.ladiff_vae_losses(*(t.data_ptr() for t in a), B, F, C, J, T, 1.0, 0.5, 1e-4, o["batch"], buf.data_ptr() + 32 * 8, ws, nb,
                                   _lib.stream_ptr())
    wsb = L.ladiff_vae_losses_workspace_bytes(B, F, C, J, T)
    assert wsb > 0 and wsb % 8 == 0
    outs = {"batch": Out(8, 1, dtype=torch.int32)}                 # four fp64 values as eight words
    refused = run_in_guards(call, wsb - 4, outs, FILLS["nan"])
    assert_refused(refused, f"ladiff_vae_losses {shape}, workspace 4 bytes short")
    assert torch.equal(state["acc"][32:36].cpu(), preset)
    for extra in (0, 1 << 20):
        res = run_fills(call, wsb, outs, ws_extra_bytes=extra)
        rep = assert_contract(res, {}, 0.0, f"ladiff_vae_losses {shape}")
        assert rep["identical"] and rep["deterministic"] and rep["guards"] == 0
        got = res["nan"]["outputs"]["batch"].reshape(-1).contiguous().view(torch.float64)
        assert rel(got.numpy(), want) < SUM_RTOL
        acc = state["acc"].cpu()                                    # of the last run (the +inf fill)
        assert torch.equal(acc[32:36], preset + got) and bool((acc[:32] == -7.25).all()) and bool((acc[36:] == -7.25).all())
    # the query is non-decreasing in every argument (host arithmetic)
    q = L.ladiff_vae_losses_workspace_bytes
    assert q(1, 1, 1, 1, 1) > 0
    for i in range(5):
        lo = [2, 30, 251, 21, 2]
        hi = list(lo); hi[i] = lo[i] * 9
        assert q(*hi) >= q(*lo)
    assert q(512, 224, 263, 22, 8) == q(256, 224, 263, 22, 8)       # the workgroup count is capped
    fake = ctypes.c_void_p(0x1000)
    assert L.ladiff_vae_losses(fake, fake, fake, fake, fake, fake, 0, 1, 1, 1, 1, 1.0, 1.0, 1.0, fake, fake, fake, 1 << 20, None) == -2
    assert L.ladiff_vae_losses(fake, fake, fake, fake, fake, fake, 1, 1, 1, 1, 1, 1.0, 1.0, 1.0, ctypes.c_void_p(0x1004), fake, fake, 1 << 20, None) == -2
    assert L.ladiff_vae_losses(None, fake, fake, fake, fake, fake, 1, 1, 1, 1, 1, 1.0, 1.0, 1.0, fake, fake, fake, 1 << 20, None) == -1
