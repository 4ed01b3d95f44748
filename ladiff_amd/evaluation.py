"""The test protocol of the reference's `test.py` around `LADIFF` (`test.py:134-157`, `base.py:55`, `ladiff.py:1386-1487`): per
replication one TM2T pass (R-precision, FID, matching score, diversity) and one multimodality pass, then mean and 95 % confidence
interval over the replications.  Batches are plain dicts with the reference's batch keys (`text`, `length`, `motion`, `word_embs`,
`pos_ohot`, `text_len`); there is no dataset code here.
"""
import numpy as np

from .evaluators import MMMetrics, TM2TMetrics


def get_metric_statistics(values, replication_times):
    """Mean over the replications (axis 0) and the half-width of the 95 % interval, 1.96 * population std / sqrt(replication_times)
    (`test.py:32-36`)."""
    values = np.asarray(values, dtype=np.float64)
    return values.mean(axis=0), 1.96 * values.std(axis=0) / np.sqrt(replication_times)


def evaluate(model, tm2t_batches, mm_batches, replication_times=1, metrics=None, joint_metrics=None):
    """Run the protocol on `model` (a `LADIFF` with evaluators set, or anything with its `t2m_eval(batch)` / `mm_eval(batch)`).

    Per replication, in the reference's order: every batch of `tm2t_batches` through `t2m_eval` into `TM2TMetrics.update(lat_t, lat_rm,
    lat_m, length)`, `compute()`; then every batch of `mm_batches` (the reference's MM loader: one prompt per batch; more are packed by
    `mm_eval`) through `mm_eval` into `MMMetrics.update(lat_rm, lengths)`, `compute()`; the two dicts merged.  Both iterables are walked
    once per replication (lists, DataLoaders; not one-shot generators).  `metrics` = (TM2TMetrics, MMMetrics) objects to use, reset
    before every replication like the reference's per-epoch reset; default-constructed when None.  `mm_batches` None or empty: no
    multimodality pass.  `joint_metrics` = an iterable of joint-space metric objects (`ComputeMetrics` / `TemosMetric`, `MRMetrics`:
    the other classes of the reference's `METRIC.TYPE`), each reset per replication, updated in the TM2T pass with `(joints_rst,
    joints_ref, batch["length"])` (`ladiff.py:1443-1445, 1464-1466`) and its `compute()` merged into the replication's values; None:
    none.

    Returns (stats, per_replication): stats[name] = (mean, conf_interval) from `get_metric_statistics`, per_replication[name] = the list
    of `replication_times` values."""
    if replication_times < 1:
        raise ValueError("replication_times must be >= 1")
    tm2t, mm = metrics if metrics is not None else (TM2TMetrics(), MMMetrics())
    joint_metrics = list(joint_metrics) if joint_metrics is not None else []
    all_metrics = {}
    for _ in range(replication_times):
        tm2t.reset()
        for jm in joint_metrics:
            jm.reset()
        for batch in tm2t_batches:
            rs = model.t2m_eval(batch)
            tm2t.update(rs["lat_t"], rs["lat_rm"], rs["lat_m"], batch["length"])
            for jm in joint_metrics:
                jm.update(rs["joints_rst"], rs["joints_ref"], batch["length"])
        values = dict(tm2t.compute(sanity_flag=False))
        for jm in joint_metrics:
            values.update(jm.compute(sanity_flag=False))
        if mm_batches is not None and mm is not None:
            mm.reset()
            seen = False
            for batch in mm_batches:
                rs = model.mm_eval(batch)
                mm.update(rs["lat_rm"], rs["lengths"])
                seen = True
            if seen:
                values.update(mm.compute(sanity_flag=False))
        for key, value in values.items():
            all_metrics.setdefault(key, []).append(float(value))
    stats = {}
    for key, items in all_metrics.items():
        mean, conf = get_metric_statistics(np.array(items), replication_times)
        stats[key] = (float(mean), float(conf))
    return stats, all_metrics


def validate(model, batches, losses=None, *, stage="vae"):
    """The validation quantities of `allsplit_step` in the reference (ladiff.py:1388-1412): every batch through the stage's training
    forward into `losses.update(rs_set)`, then `losses.compute()` - the mean over the batches of each loss.
    stage "vae" (the default): `model.train_vae_forward` into an `MLDLosses` - {recons_feature, recons_joints, kl_motion, total, ...}.
    stage "diffusion", or a `DiffusionLosses` passed in: `model.train_diffusion_forward` (random timesteps, noise and text drop, as the
    reference's validation step draws them) into a `DiffusionLosses` - {inst_loss, x_loss, total}.
    `losses` = the object to use (NOT reset here: a caller may accumulate over several calls); default-constructed from `model.cfg`."""
    from .losses import DiffusionLosses, MLDLosses
    if isinstance(losses, DiffusionLosses):
        stage = "diffusion"
    if stage not in ("vae", "diffusion"):
        raise ValueError(f"stage {stage!r} not supported")
    if losses is None:
        cls = DiffusionLosses if stage == "diffusion" else MLDLosses
        kw = {} if stage == "diffusion" else {"stage": "vae"}
        losses = cls(vae=getattr(model, "is_vae", True), cfg=getattr(model, "cfg", None), **kw)
    forward = model.train_diffusion_forward if stage == "diffusion" else model.train_vae_forward
    for batch in batches:
        losses.update(forward(batch))
    return losses.compute()
