"""The reference's `MLDLosses` (models/losses/mld.py) in stage "vae" on the GPU: the stage-1 validation quantities `recons_feature`,
`recons_joints`, `kl_motion` and `total`, fed with the `rs_set` of `LADIFF.train_vae_forward` (ladiff.py:815-871).  `update()` queues two
launches (`ladiff_vae_losses`: per-workgroup fp64 partial sums, then one workgroup adds them, divides and adds the four values to an fp64
accumulator on the device - the reference's `+=` per update) and returns the batch's `total` as a 0-dim device tensor without
synchronising; `compute()` copies the accumulator once and divides by the update count.  There is no CPU implementation.

Stage "diffusion" is `DiffusionLosses` below: `inst_loss` (the noise-prediction MSE of `LADIFF.train_diffusion_forward`'s `n_set`) and
`total`, through `ladiff_diffusion_losses`, with the same interface.
"""
import numpy as np
import torch

from . import _lib
from .pipeline import _cfg_get

# the reference's state names in stage "vae", in its order (mld.py:39-55); the ones its update() never touches in this stage stay 0
VAE_STAGE_LOSSES = ("recons_feature", "recons_verts", "recons_joints", "recons_limb", "gen_feature", "gen_joints", "kl_motion", "total")
_COMPUTED = ("recons_feature", "recons_joints", "kl_motion", "total")      # layout of the device accumulator


class MLDLosses:
    """`MLDLosses(vae, mode, cfg)` of the reference, stage "vae".  The lambdas come from `cfg.LOSS` (`LAMBDA_REC`, `LAMBDA_JOINT`,
    `LAMBDA_KL`) when `cfg` is given: a `recons_*` loss takes `LAMBDA_REC`, `kl_motion` takes `LAMBDA_KL`, and a loss whose name ends in
    `joints` takes `LAMBDA_JOINT` whatever its family (mld.py:81-96)."""

    def __init__(self, vae=True, mode="xyz", cfg=None, *, stage=None, lambda_rec=1.0, lambda_joint=1.0, lambda_kl=1e-4):
        if stage is None:
            stage = _cfg_get(_cfg_get(cfg, "TRAIN"), "STAGE", "vae")
        if stage not in ("vae", "diffusion", "vae_diffusion"):
            raise ValueError(f"Stage {stage} not supported")
        if stage != "vae":
            raise NotImplementedError(f'MLDLosses(stage={stage!r}) is not built: this class holds the stage-"vae" losses; the stage-'
                                      '"diffusion" losses are DiffusionLosses')
        if _cfg_get(_cfg_get(_cfg_get(cfg, "TRAIN"), "ABLATION"), "JOINT_DISTRO_FIX", False):
            raise NotImplementedError("MLDLosses with JOINT_DISTRO_FIX (KLLossMulti) is not built")
        self.vae, self.mode, self.cfg, self.stage = vae, mode, cfg, stage
        loss_cfg = _cfg_get(cfg, "LOSS")
        lam = {"recons": float(_cfg_get(loss_cfg, "LAMBDA_REC", lambda_rec)), "kl": float(_cfg_get(loss_cfg, "LAMBDA_KL", lambda_kl)),
               "gen": float(_cfg_get(loss_cfg, "LAMBDA_GEN", 1.0))}
        self.losses = list(VAE_STAGE_LOSSES)
        self._params = {}
        for loss in self.losses[:-1]:
            self._params[loss] = lam[loss.split("_")[0]]
            if loss.split("_")[-1] == "joints":                       # mld.py:95-96
                self._params[loss] = float(_cfg_get(loss_cfg, "LAMBDA_JOINT", lambda_joint))
        self.reset()

    def reset(self):
        self.count = 0
        self._host = np.zeros(len(_COMPUTED), dtype=np.float64)    # sums merged in by add_sums / folded from another device
        self._acc = None                                           # fp64 [4] on the device the updates run on
        self.last_batch = None                                     # fp64 [4] device tensor of the latest update

    def update(self, rs_set):
        """One batch: `m_rst` / `m_ref` [B,F,C], `joints_rst` / `joints_ref` [B,F,J,3], `dist_m` = Normal(mu, std) [T,B,256]; `dist_ref`
        must be the standard normal (`model.vae: true`, ladiff.py:851-854).  Returns the weighted `total` of the batch."""
        m_rst, m_ref, j_rst, j_ref, dist = (rs_set[k] for k in ("m_rst", "m_ref", "joints_rst", "joints_ref", "dist_m"))
        ref = rs_set.get("dist_ref")
        # train_vae_forward marks the standard normal it builds; a foreign object is looked at (one host synchronisation)
        if ref is None or ref is dist or ref.loc.shape != dist.loc.shape or not (
                getattr(ref, "_ladiff_standard_normal", False) or not (bool(ref.loc.any()) or bool((ref.scale != 1).any()))):
            raise NotImplementedError("kl_motion is built against the standard normal only (dist_ref of model.vae: true)")
        if m_rst.dim() != 3 or m_rst.shape != m_ref.shape:
            raise _lib.LadiffHipError(f"m_rst / m_ref must be two [B,F,C] tensors, got {tuple(m_rst.shape)} and {tuple(m_ref.shape)}")
        B, F, C = m_rst.shape
        if j_rst.dim() != 4 or j_rst.shape != j_ref.shape or tuple(j_rst.shape[:2]) != (B, F) or j_rst.shape[-1] != 3:
            raise _lib.LadiffHipError(f"joints must be two [{B},{F},J,3] tensors, got {tuple(j_rst.shape)} and {tuple(j_ref.shape)}")
        J = j_rst.shape[2]
        mu, std = dist.loc, dist.scale
        if mu.dim() != 3 or mu.shape != std.shape or mu.shape[1] != B or mu.shape[2] != 256:
            raise _lib.LadiffHipError(f"dist_m must be Normal over [T,{B},256], got {tuple(mu.shape)}")
        T = mu.shape[0]
        device = next((t.device for t in (m_rst, m_ref, j_rst, j_ref, mu) if t.is_cuda), None)
        if device is None:
            if not torch.cuda.is_available():
                raise _lib.LadiffHipError("the losses run on the GPU only; got CPU tensors and there is no GPU (no CPU fallback exists)")
            device = torch.device("cuda", torch.cuda.current_device())
        L = _lib.lib()
        with torch.cuda.device(device):
            a = [t.detach().to(device=device, dtype=torch.float32).contiguous() for t in (m_rst, m_ref, j_rst, j_ref, mu, std)]
            if self._acc is not None and self._acc.device != device:
                self._host += self._acc.cpu().numpy()
                self._acc = None
            if self._acc is None:
                self._acc = torch.zeros(len(_COMPUTED), dtype=torch.float64, device=device)
            batch = torch.empty(len(_COMPUTED), dtype=torch.float64, device=device)
            wsb = L.ladiff_vae_losses_workspace_bytes(B, F, C, J, T)
            ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device=device)
            _lib.check(L.ladiff_vae_losses(*(t.data_ptr() for t in a), B, F, C, J, T, self._params["recons_feature"],
                                           self._params["recons_joints"], self._params["kl_motion"], batch.data_ptr(), self._acc.data_ptr(),
                                           ws.data_ptr(), wsb, torch.cuda.current_stream(device).cuda_stream))
        self.last_batch = batch
        self.count += 1
        return batch[3]

    def sums(self):
        """{"count", "sums"}: the update count and the fp64 sums [recons_feature, recons_joints, kl_motion, total] as a numpy array
        (waits for the queued updates)."""
        total = self._host.copy()
        if self._acc is not None:
            total += self._acc.cpu().numpy()
        return {"count": self.count, "sums": total}

    def add_sums(self, other):
        """Merge another object's state (its `sums()` dict, or the object): the reference's dist_reduce_fx="sum"."""
        other = other.sums() if hasattr(other, "sums") else other
        add = np.asarray(other["sums"], dtype=np.float64)
        if add.shape != self._host.shape:
            raise ValueError(f"sums of {add.shape[0]} values merged into {self._host.shape[0]}")
        self._host += add
        self.count += int(other["count"])

    def compute(self, split=None):
        """{loss: sum / count} over the reference's stage-"vae" names (mld.py:137-139); the ones this stage never updates are 0.0."""
        st = self.sums()
        out = {loss: 0.0 for loss in self.losses}
        with np.errstate(divide="ignore", invalid="ignore"):
            for name, s in zip(_COMPUTED, st["sums"]):
                out[name] = float(s / np.float64(st["count"]))
        return out

    def loss2logname(self, loss, split):
        if loss == "total":
            return f"{loss}/{split}"
        loss_type, name = loss.split("_")
        return f"{loss_type}/{name}/{split}"


# the reference's state names in stage "diffusion" with LAMBDA_PRIOR == 0, in its order (mld.py:30-36, :53)
DIFFUSION_STAGE_LOSSES = ("inst_loss", "x_loss", "total")
_DIFF_COMPUTED = ("inst_loss", "total")                                     # layout of the device accumulator


class DiffusionLosses:
    """`MLDLosses(vae, mode, cfg)` of the reference in stage "diffusion" (mld.py:30-36, :108-120): `inst_loss` = `nn.MSELoss` of
    `noise_pred` against `noise` over every element, padded latent rows included, and `total` = 1 x `inst_loss` (mld.py:67-69).  `x_loss`
    belongs to `PREDICT_EPSILON: False` and stays 0.0; that branch and the prior loss (`LOSS.LAMBDA_PRIOR != 0`) are not built.  Same
    interface and the same device-side accumulation as `MLDLosses`."""

    def __init__(self, vae=True, mode="xyz", cfg=None, *, predict_epsilon=None, lambda_prior=None):
        abl = _cfg_get(_cfg_get(cfg, "TRAIN"), "ABLATION")
        if predict_epsilon is None:
            predict_epsilon = _cfg_get(abl, "PREDICT_EPSILON", True)
        if lambda_prior is None:
            lambda_prior = _cfg_get(_cfg_get(cfg, "LOSS"), "LAMBDA_PRIOR", 0.0)
        if not predict_epsilon:
            raise NotImplementedError("DiffusionLosses with PREDICT_EPSILON: False (x_loss) is not built")
        if float(lambda_prior) != 0.0:
            raise NotImplementedError("DiffusionLosses with LAMBDA_PRIOR != 0 (prior_loss) is not built")
        self.vae, self.mode, self.cfg, self.stage = vae, mode, cfg, "diffusion"
        self.losses = list(DIFFUSION_STAGE_LOSSES)
        self._params = {"inst_loss": 1.0, "x_loss": 1.0}                    # mld.py:67-72
        self.reset()

    def reset(self):
        self.count = 0
        self._host = np.zeros(len(_DIFF_COMPUTED), dtype=np.float64)
        self._acc = None                                                    # fp64 [2] on the device the updates run on
        self.last_batch = None                                              # fp64 [2] device tensor of the latest update

    def update(self, rs_set):
        """One batch: `noise_pred` and `noise`, two tensors of one shape (`_diffusion_process`'s `n_set`).  Returns the batch's `total`."""
        pred, noise = rs_set["noise_pred"], rs_set["noise"]
        if not torch.is_tensor(pred) or not torch.is_tensor(noise) or pred.shape != noise.shape or pred.numel() == 0:
            raise _lib.LadiffHipError("noise_pred / noise must be two non-empty tensors of one shape")
        device = next((t.device for t in (pred, noise) if t.is_cuda), None)
        if device is None:
            if not torch.cuda.is_available():
                raise _lib.LadiffHipError("the losses run on the GPU only; got CPU tensors and there is no GPU (no CPU fallback exists)")
            device = torch.device("cuda", torch.cuda.current_device())
        L = _lib.lib()
        with torch.cuda.device(device):
            a, b = (t.detach().to(device=device, dtype=torch.float32).contiguous() for t in (pred, noise))
            if self._acc is not None and self._acc.device != device:
                self._host += self._acc.cpu().numpy()
                self._acc = None
            if self._acc is None:
                self._acc = torch.zeros(len(_DIFF_COMPUTED), dtype=torch.float64, device=device)
            batch = torch.empty(len(_DIFF_COMPUTED), dtype=torch.float64, device=device)
            wsb = L.ladiff_diffusion_losses_workspace_bytes(a.numel())
            ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device=device)
            _lib.check(L.ladiff_diffusion_losses(a.data_ptr(), b.data_ptr(), a.numel(), self._params["inst_loss"], batch.data_ptr(),
                                                 self._acc.data_ptr(), ws.data_ptr(), wsb, torch.cuda.current_stream(device).cuda_stream))
        self.last_batch = batch
        self.count += 1
        return batch[1]

    def sums(self):
        """{"count", "sums"}: the update count and the fp64 sums [inst_loss, total] as a numpy array (waits for the queued updates)."""
        total = self._host.copy()
        if self._acc is not None:
            total += self._acc.cpu().numpy()
        return {"count": self.count, "sums": total}

    add_sums = MLDLosses.add_sums
    loss2logname = MLDLosses.loss2logname

    def compute(self, split=None):
        """{loss: sum / count} over the reference's stage-"diffusion" names (mld.py:137-139); `x_loss` is 0.0."""
        st = self.sums()
        out = {loss: 0.0 for loss in self.losses}
        with np.errstate(divide="ignore", invalid="ignore"):
            for name, s in zip(_DIFF_COMPUTED, st["sums"]):
                out[name] = float(s / np.float64(st["count"]))
        return out
