#!/usr/bin/env python3
"""Golden vectors for the stage-1 (LA-VAE) path from the REFERENCE modules (build container only; see make_golden.py): `LADiffVae.encode`
with DVAE=True, PERCENTAGE_NOISED=0.33 -> `decode`, and the reference-side stage-"vae" losses of that reconstruction.

`vae.add_noise` is replaced by a wrapper that calls the original on `zeros_like(x)` - which returns the exact noise field - records the
field and returns `x + field`, the operation the original performs.  The field is stored as (`positions`, `values`): the distinct
corrupted positions of the flattened [F, C] block and each sample's value there."""
import os, sys
import numpy as np
import torch
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                     # noqa: E402  (reference module builders + ABL; puts the reference on sys.path)
from ladiff.data.humanml.scripts.motion_process import recover_from_ric   # noqa: E402

torch.set_num_threads(8)
mg.ABL.DVAE, mg.ABL.PERCENTAGE_NOISED = True, 0.33
with torch.no_grad():
    for name, C, J, lens in (("vae_stage_humanml", 263, 22, [24, 49, 60]), ("vae_stage_kit", 251, 21, [33, 7])):
        vae = mg.build_vae(C)
        assert vae.dvae and vae.percentage_noised == 0.33
        rs = np.random.RandomState(91 + C)
        F = max(lens)
        feats = torch.from_numpy(rs.standard_normal((len(lens), F, C)).astype(np.float32))
        for i, l in enumerate(lens):
            feats[i, l:] = 0                                     # padding frames zero
        mean = torch.from_numpy((0.1 * rs.standard_normal(C)).astype(np.float32))
        std_f = torch.from_numpy((0.05 + 0.2 * rs.random_sample(C)).astype(np.float32))
        seen = {}
        original = vae.add_noise

        def add_noise(x):
            field = original(torch.zeros_like(x))
            seen["field"] = field
            return x + field

        vae.add_noise = add_noise
        np.random.seed(17 + C)
        torch.manual_seed(9)
        latent, dist, counts = vae.encode(feats, lens)
        mu, std = dist.loc, dist.scale
        eps = (latent - mu) / std                               # the draw rsample() made (valid rows)
        for i, c in enumerate(counts.tolist()):
            eps[c:, i] = 0
        field = seen["field"].reshape(len(lens), F * C)
        positions = torch.nonzero((field != 0).any(dim=0)).flatten()
        values = field[:, positions]
        back = torch.zeros_like(field)
        back[:, positions] = values
        assert torch.equal(back, field)
        m_rst = vae.decode(latent, lens)
        joints_rst = recover_from_ric(m_rst * std_f + mean, J)   # = datamodule.feats2joints, as make_golden_feats2joints.py
        joints_ref = recover_from_ric(feats * std_f + mean, J)
        smooth = torch.nn.SmoothL1Loss(reduction="mean")
        ref = torch.distributions.Normal(torch.zeros_like(mu), torch.ones_like(std))
        out = dict(features=feats, lengths=np.array(lens), positions=positions, values=values, eps=eps, counts=counts, mu=mu, std=std,
                   latent=latent, m_rst=m_rst, mean=mean, std_feats=std_f, njoints=np.int64(J),
                   recons_feature=smooth(m_rst, feats), recons_joints=smooth(joints_rst, joints_ref),
                   kl_motion=torch.distributions.kl_divergence(dist, ref).mean())
        mg.save(name, **out)
        d = (m_rst - feats).abs()
        print(name, "counts", counts.tolist(), "positions", positions.numel(), "of", int(F * C * 0.33), "draws; |d| >= 1:",
              f"{(d >= 1).float().mean().item():.2f}", "sigma", f"{std.min().item():.2f} .. {std.max().item():.2f}")
