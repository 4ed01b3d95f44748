#!/usr/bin/env python3
"""Golden features for joints2feats from the REFERENCE's own `process_file` (data/humanml/scripts/motion_process.py:169-351).  Run where
the reference is checked out: `python tests/golden/make_golden_joints2feats.py path/to/reference` (needs scipy, which the reference's
skeleton.py imports for the forward vector's gaussian filter).

The reference's files are loaded one by one (common/quaternion.py, common/skeleton.py, utils/paramUtil.py, scripts/motion_process.py)
under their own module names with empty parent packages.  `process_file` reads module globals that only the script's `__main__` block
defines (motion_process.py:435-460: tgt_offsets, n_raw_offsets, kinematic_chain, face_joint_indx, fid_r, fid_l, l_idx1, l_idx2); they
are injected here with the HumanML3D values of that block.  The call is `process_file(positions, 0.002)` as at :468 - NOT
`HumanML3DDataModule.joints2feats`, which passes njoints where feet_thre belongs.

tests/golden/joints2feats_humanml.npz holds arrays only: the target pose and its offsets (`Skeleton.get_offsets_joints`), and per
L in {2, 3, 40, 82, 197} the input (float64, tests/joints2feats_ref.motion at that length's seed) and the features [L - 1, 263] once
with the uniform-skeleton step (`feats_tgt_L`) and once with that step replaced by the identity (`feats_raw_L`).  Every feature the
reference returns is a float32 value held in a float64 array (its quaternion helpers work in float32); the script checks that and
stores float32."""
import importlib.util, os, sys, types
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
SRC = os.path.join(sys.argv[1], "src", "ladiff")
sys.path.insert(0, os.path.dirname(HERE))
import joints2feats_ref as ref                                              # noqa: E402  (inputs only)


def _package(name):
    mod = types.ModuleType(name)
    mod.__path__ = []
    sys.modules[name] = mod


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(SRC, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


for pkg in ("ladiff", "ladiff.data", "ladiff.data.humanml", "ladiff.data.humanml.common", "ladiff.data.humanml.utils",
            "ladiff.data.humanml.scripts"):
    _package(pkg)
_load("ladiff.data.humanml.common.quaternion", "data/humanml/common/quaternion.py")
skel = _load("ladiff.data.humanml.common.skeleton", "data/humanml/common/skeleton.py")
par = _load("ladiff.data.humanml.utils.paramUtil", "data/humanml/utils/paramUtil.py")
mp = _load("ladiff.data.humanml.scripts.motion_process", "data/humanml/scripts/motion_process.py")

# the globals of motion_process.py:435-460 (HumanML3D)
mp.l_idx1, mp.l_idx2 = 5, 8
mp.fid_r, mp.fid_l = [8, 11], [7, 10]
mp.face_joint_indx = [2, 1, 17, 16]
mp.n_raw_offsets = torch.from_numpy(par.t2m_raw_offsets)
mp.kinematic_chain = par.t2m_kinematic_chain
pose = ref.target_pose()
mp.tgt_offsets = skel.Skeleton(mp.n_raw_offsets, mp.kinematic_chain, "cpu").get_offsets_joints(torch.from_numpy(pose))
uniform = mp.uniform_skeleton

out = {"target_pose": pose, "tgt_offsets": mp.tgt_offsets.numpy().astype(np.float32)}
for L in (2, 3, 40, 82, 197):
    x = ref.motion(L, ref.CASE_SEEDS[L])
    out[f"x_{L}"] = x
    for tag, fn in (("tgt", uniform), ("raw", lambda positions, target: positions)):
        mp.uniform_skeleton = fn
        feats = mp.process_file(x.copy(), 0.002)[0]
        assert feats.shape == (L - 1, 263) and np.isfinite(feats).all()
        assert (feats.astype(np.float32).astype(np.float64) == feats).all()
        out[f"feats_{tag}_{L}"] = feats.astype(np.float32)
path = os.path.join(HERE, "joints2feats_humanml.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes")
