"""fp64 numpy restatements of the stage-"vae" losses (`MLDLosses` in stage "vae", models/losses/mld.py:81-96, :98-107, :157-164) and of
the DVAE corruption scatter (`LADiffVae.add_noise`, ladiff_vae.py:136-150): what the device results of `ladiff_vae_losses` and
`ladiff_vae_encode_dvae` are held against.  TEST INFRASTRUCTURE ONLY (a plain helper module, like joint_metrics_ref.py)."""
import numpy as np


def _f64(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)


def smooth_l1(rst, ref):
    """torch.nn.SmoothL1Loss(reduction='mean'), beta 1: mean of 0.5 d^2 where |d| < 1, |d| - 0.5 elsewhere."""
    d = _f64(rst) - _f64(ref)
    ad = np.abs(d)
    return float(np.where(ad < 1.0, 0.5 * d * d, ad - 0.5).mean())


def kl_standard_normal(mu, std):
    """mean of torch.distributions.kl_divergence(Normal(mu, std), Normal(0, 1)) = 0.5 (std^2 + mu^2 - 1 - log std^2), every element."""
    m, v = _f64(mu), _f64(std) ** 2
    return float((0.5 * (v + m * m - 1.0 - np.log(v))).mean())


def losses(m_rst, m_ref, joints_rst, joints_ref, mu, std, lambda_rec=1.0, lambda_joint=1.0, lambda_kl=1e-4):
    """[recons_feature, recons_joints, kl_motion, total] as float64."""
    rf, rj, kl = smooth_l1(m_rst, m_ref), smooth_l1(joints_rst, joints_ref), kl_standard_normal(mu, std)
    return np.array([rf, rj, kl, lambda_rec * rf + lambda_joint * rj + lambda_kl * kl], dtype=np.float64)


def corrupt(features, positions, values):
    """features [B,F,C] + the noise field that holds values[b, k] at flat position positions[k] of sample b's [F, C] block (distinct
    positions), zero elsewhere; in the features' own dtype (one fp32 addition per corrupted element, as `x + noise`)."""
    x = np.array(features.detach().cpu().numpy() if hasattr(features, "detach") else features, copy=True)
    B = x.shape[0]
    field = np.zeros((B, x.shape[1] * x.shape[2]), dtype=x.dtype)
    pos = np.asarray(positions.cpu().numpy() if hasattr(positions, "cpu") else positions, dtype=np.int64)
    field[:, pos] = np.asarray(values.detach().cpu().numpy() if hasattr(values, "detach") else values, dtype=x.dtype)
    return x + field.reshape(x.shape)
