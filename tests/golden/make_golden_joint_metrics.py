#!/usr/bin/env python3
"""Golden values for the joint-space metrics from the REFERENCE's own `ComputeMetrics` (models/metrics/compute.py) and `MRMetrics`
(models/metrics/mr.py).  Run where the reference is checked out: `python tests/golden/make_golden_joint_metrics.py path/to/reference`.

The reference's files are loaded one by one (metrics/utils.py, compute.py, mr.py, transforms/joints2jfeats/*.py, utils/joints.py,
utils/geometry.py, models/tools/tools.py for `remove_padding`) under their own module names, with empty parent packages and a few-line
stand-in for `torchmetrics.Metric` (`add_state` -> `setattr`), so neither torchmetrics nor smplx is needed (and an empty
`ladiff.utils.rotation_conversions`, which geometry.py imports for functions not used here).

tests/golden/joint_metrics.npz holds arrays only.  Per case: the inputs (float32), the lengths, the eight part indices read off the
reference's joint-name lists, and - once from the float32 inputs and once from the same inputs as float64 - the reference's `compute()`
values and its per-sequence contributions (the state after an update with that sequence alone).  In the float64 pass the default
dtype is float64 (the classes' state and `torch.eye` follow it) and `calc_pampjpe`'s `.float()` casts are left out: the function is
restated here as the same two calls of the reference (`batch_compute_similarity_transform_torch`, `compute_mpjpe`) without them."""
import importlib.util, os, sys, types
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
SRC = os.path.join(sys.argv[1], "src", "ladiff")


class _Metric:
    def __init__(self, **kwargs):
        pass

    def add_state(self, name, default, dist_reduce_fx=None):
        setattr(self, name, default.clone())


def _package(name):
    mod = types.ModuleType(name)
    mod.__path__ = []
    sys.modules[name] = mod
    return mod


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(SRC, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


sys.modules["torchmetrics"] = types.ModuleType("torchmetrics")
sys.modules["torchmetrics"].Metric = _Metric
for pkg in ("ladiff", "ladiff.models", "ladiff.models.tools", "ladiff.models.metrics", "ladiff.transforms", "ladiff.transforms.joints2jfeats",
            "ladiff.utils", "ladiff.utils.rotation_conversions"):          # the last: imported by geometry.py, unused here
    _package(pkg)
jmod = _load("ladiff.utils.joints", "utils/joints.py")
_load("ladiff.utils.geometry", "utils/geometry.py")
_load("ladiff.models.tools.tools", "models/tools/tools.py")
_load("ladiff.transforms.joints2jfeats.base", "transforms/joints2jfeats/base.py")
_load("ladiff.transforms.joints2jfeats.tools", "transforms/joints2jfeats/tools.py")
sys.modules["ladiff.transforms.joints2jfeats"].Rifke = _load("ladiff.transforms.joints2jfeats.rifke", "transforms/joints2jfeats/rifke.py").Rifke
mutil = _load("ladiff.models.metrics.utils", "models/metrics/utils.py")
cmod = _load("ladiff.models.metrics.compute", "models/metrics/compute.py")
mrmod = _load("ladiff.models.metrics.mr", "models/metrics/mr.py")
_pampjpe_float = mrmod.calc_pampjpe


def _pampjpe_keep_dtype(preds, target):
    hat, _ = mutil.batch_compute_similarity_transform_torch(preds, target)
    return mutil.compute_mpjpe(hat, target, sample_wise=True)


# a standing figure about 0.9 high at the root, by joint name (both name lists; "TOP" fills a 22nd joint of the 21-name mmm list)
REST = {"root": (0, .9, 0), "RH": (-.09, .85, 0), "LH": (.09, .85, 0), "BP": (0, 1.0, .01), "RK": (-.1, .48, .03), "LK": (.1, .48, .03),
        "BT": (0, 1.15, .02), "RMrot": (-.1, .08, -.03), "LMrot": (.1, .08, -.03), "BLN": (0, 1.3, .01), "RF": (-.11, .02, .1),
        "LF": (.11, .02, .1), "BMN": (0, 1.42, .02), "RSI": (-.07, 1.36, .01), "LSI": (.07, 1.36, .01), "BUN": (0, 1.55, .04),
        "RS": (-.18, 1.38, 0), "LS": (.18, 1.38, 0), "RE": (-.25, 1.12, -.02), "LE": (.25, 1.12, -.02), "RW": (-.27, .87, .06),
        "LW": (.27, .87, .06), "RA": (-.1, .09, -.05), "LA": (.1, .09, -.05), "TOP": (0, 1.65, .03)}
PART_NAMES = ("LS", "RS", "LH", "RH", "LMrot", "RMrot", "LF", "RF")
QUANT = 2.0 ** -14                                   # inputs on a 2^-14 grid: exact in float32, and the file compresses


def motion(rs, names, B, F):
    """ref = the rest pose turned by a random-walk heading (started near pi, so that atan2 wraps) on a random-walk root, plus small
    per-joint noise; rst = ref + noise.  Every one of the F frames, the padded ones too, holds such a pose, different in rst and ref."""
    rest = np.array([REST[n] for n in names], dtype=np.float64)
    rest = rest - rest[0]
    yaw = 2.9 + np.cumsum(rs.standard_normal((B, F)) * 0.05, axis=1)
    c, s = np.cos(yaw)[..., None], np.sin(yaw)[..., None]
    body = np.stack([rest[:, 0] * c + rest[:, 2] * s, np.broadcast_to(rest[:, 1], c.shape[:2] + (len(names),)),
                     -rest[:, 0] * s + rest[:, 2] * c], axis=-1)                                   # [B,F,J,3]
    root = np.cumsum(rs.standard_normal((B, F, 3)) * np.array([0.02, 0.004, 0.02]), axis=1) + np.array([0.3, 0.9, -0.2])
    ref = body + root[:, :, None, :] + rs.standard_normal(body.shape) * 0.01
    rst = ref + rs.standard_normal(body.shape) * 0.02 + np.cumsum(rs.standard_normal((B, F, 1, 3)) * 0.003, axis=1)
    q = lambda v: (np.round(v / QUANT) * QUANT).astype(np.float32)
    return q(rst), q(ref)


def run(rst, ref, lengths, jointstype, dtype):
    """compute() values and per-sequence contributions of both classes at `dtype`."""
    torch.set_default_dtype(dtype)
    mrmod.calc_pampjpe = _pampjpe_float if dtype == torch.float32 else _pampjpe_keep_dtype
    J = rst.shape[2]
    a, b = torch.from_numpy(rst).to(dtype), torch.from_numpy(ref).to(dtype)
    out = {}
    for tag, make in (("ape", lambda: cmod.ComputeMetrics(njoints=J, jointstype=jointstype)),
                      ("mr", lambda: mrmod.MRMetrics(njoints=J, jointstype=jointstype))):
        m = make()
        m.update(a, b, list(lengths))
        values = m.compute(sanity_flag=False)
        out[tag + "_keys"] = list(values)
        out[tag + "_compute"] = np.array([float(v) for v in values.values()], dtype=np.float64)
        rows = []
        for i, n in enumerate(lengths):
            one = make()
            one.update(a[i:i + 1], b[i:i + 1], [n])
            rows.append(np.concatenate([np.atleast_1d(getattr(one, name).numpy().astype(np.float64)) for name in one.metrics]))
        out[tag + "_rows"] = np.stack(rows)
    torch.set_default_dtype(torch.float32)
    mrmod.calc_pampjpe = _pampjpe_float
    return out


def conditioning(rst, ref):
    """The two conditions under which the reference's own PA-MPJPE is well-conditioned: sigma3 / sigma1 of every frame's K, var1."""
    x1 = rst.astype(np.float64).reshape(-1, rst.shape[2], 3)
    x2 = ref.astype(np.float64).reshape(-1, ref.shape[2], 3)
    x1, x2 = x1 - x1.mean(axis=1, keepdims=True), x2 - x2.mean(axis=1, keepdims=True)
    sv = np.linalg.svd(np.einsum("nja,njb->nab", x1, x2), compute_uv=False)
    return (sv[:, 2] / sv[:, 0]).min(), (x1 ** 2).sum(axis=(1, 2)).min()


CASES = (("a", 5, 196, 22, [196, 65, 64, 2, 120], "humanml3d"), ("b", 3, 70, 21, [70, 33, 3], "humanml3d"),
         ("c", 2, 3, 22, [3, 2], "humanml3d"), ("d", 5, 196, 22, [196, 65, 64, 2, 120], "mmm"))
out = {"cases": np.array([c[0] for c in CASES])}
rs = np.random.RandomState(23)
for tag, B, F, J, lengths, jointstype in CASES:
    listed = list(jmod.mmm_joints if jointstype == "mmm" else jmod.humanml3d_joints)
    names = (listed + ["TOP"])[:J]
    rst, ref = motion(rs, names, B, F)
    ratio, var1 = conditioning(rst, ref)
    assert ratio > 1e-3 and var1 > 0, (tag, ratio, var1)
    out.update({f"{tag}_rst": rst, f"{tag}_ref": ref, f"{tag}_lengths": np.array(lengths, dtype=np.int64),
                f"{tag}_jointstype": np.array(jointstype), f"{tag}_parts": np.array([listed.index(n) for n in PART_NAMES], dtype=np.int64)})
    r64, r32 = run(rst, ref, lengths, jointstype, torch.float64), run(rst, ref, lengths, jointstype, torch.float32)
    assert r64["ape_keys"] == r32["ape_keys"] and r64["mr_keys"] == r32["mr_keys"]
    out["ape_keys"], out["mr_keys"] = np.array(r64["ape_keys"]), np.array(r64["mr_keys"])
    for kind in ("ape", "mr"):
        for what in ("compute", "rows"):
            v64, v32 = r64[f"{kind}_{what}"], r32[f"{kind}_{what}"]
            assert np.isfinite(v64).all() and np.isfinite(v32).all(), (tag, kind, what)
            out[f"{tag}_{kind}_{what}64"], out[f"{tag}_{kind}_{what}32"] = v64, v32
            print(tag, kind, what, v64.shape, "max |f32 - f64| / max |f64| =", f"{np.abs(v32 - v64).max() / np.abs(v64).max():.2e}")
    print(tag, jointstype, "sigma3/sigma1 >=", f"{ratio:.3e}", "var1 >=", f"{var1:.3e}", "parts", out[f"{tag}_parts"].tolist())
np.savez_compressed(os.path.join(HERE, "joint_metrics.npz"), **out)
print(os.path.getsize(os.path.join(HERE, "joint_metrics.npz")), "bytes")
