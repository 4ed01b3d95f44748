"""joints2feats on the GPU: joint positions -> 263-dim HumanML3D features, the direction `Feats2Joints` inverts.  The reference's
`HumanML3DDataModule.joints2feats` (HumanML3D.py:50-55) calls `process_file` (data/humanml/scripts/motion_process.py:169-351) on the CPU
in numpy; here it is one kernel (csrc/joints2feats.hip), so what `LADIFF.forward` returned can go straight back into `LADIFF.edit`."""
import torch

from . import _lib

NJOINTS, NFEATS, MAX_FRAMES = 22, 263, 256
FEET_THRE = 0.002            # the reference's data script for HumanML3D (motion_process.py:468)

# t2m skeleton (utils/paramUtil.py): parent of every joint and the unit direction of its bone in the rest pose
_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19)
_RAW_OFFSETS = ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, -1, 0), (0, 1, 0), (0, -1, 0), (0, -1, 0), (0, 1, 0), (0, 0, 1),
                (0, 0, 1), (0, 1, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, -1, 0), (0, -1, 0), (0, -1, 0), (0, -1, 0), (0, -1, 0), (0, -1, 0))


def offsets_of_pose(pose):
    """`Skeleton.get_offsets_joints` (common/skeleton.py:43-51): raw direction x bone length of a pose [22, 3], float32 [22, 3]."""
    pose = torch.as_tensor(pose).detach().cpu().to(torch.float64)
    if tuple(pose.shape) != (NJOINTS, 3):
        raise ValueError(f"target_pose must be [{NJOINTS}, 3], got {tuple(pose.shape)}")
    raw = torch.tensor(_RAW_OFFSETS, dtype=torch.float32)
    lengths = torch.stack([torch.zeros((), dtype=torch.float64)] + [torch.linalg.norm(pose[i] - pose[_PARENTS[i]]) for i in range(1, NJOINTS)])
    return raw * lengths.to(torch.float32)[:, None]


class Joints2Feats:
    """`Joints2Feats(mean, std)(joints[L,22,3]) -> features[L-1,263]`, or `(joints[B,L,22,3], lengths) -> [B,L-1,263]` with rows past
    `lengths[b] - 2` zero, on the device the joints are on.  2 <= lengths[b] <= L <= 256.  HumanML3D only (njoints = 22).

    `target_offsets` ([22,3], `Skeleton.get_offsets_joints` of the target pose) or `target_pose` ([22,3], its offsets are taken here)
    turn on the reference's uniform-skeleton step; without either the step is skipped - right for motions that are on the model's
    skeleton already, such as `LADIFF.forward`'s output.  `normalize=True` returns `(features - mean) / std`, what `LADIFF.edit`,
    `vae.encode` and the evaluators take.  No CPU implementation: CPU tensors raise."""

    def __init__(self, mean=None, std=None, njoints=NJOINTS, feet_thre=FEET_THRE, target_offsets=None, target_pose=None):
        if int(njoints) != NJOINTS:
            raise ValueError(f"joints2feats is built for the {NJOINTS}-joint HumanML3D skeleton only (the reference has no KIT form); got {njoints}")
        if (mean is None) != (std is None):
            raise ValueError("mean and std come together")
        if not float(feet_thre) > 0:
            raise ValueError("feet_thre must be positive")
        if target_offsets is not None and target_pose is not None:
            raise ValueError("give target_offsets or target_pose, not both")
        self.njoints, self.feet_thre = NJOINTS, float(feet_thre)
        self.mean = self.std = None
        if mean is not None:
            self.mean = torch.as_tensor(mean, dtype=torch.float32).detach().cpu().contiguous()
            self.std = torch.as_tensor(std, dtype=torch.float32).detach().cpu().contiguous()
            if tuple(self.mean.shape) != (NFEATS,) or tuple(self.std.shape) != (NFEATS,):
                raise ValueError(f"mean / std must be [{NFEATS}]")
        if target_pose is not None:
            target_offsets = offsets_of_pose(target_pose)
        self.target_offsets = None
        if target_offsets is not None:
            self.target_offsets = torch.as_tensor(target_offsets, dtype=torch.float32).detach().cpu().contiguous()
            if tuple(self.target_offsets.shape) != (NJOINTS, 3):
                raise ValueError(f"target_offsets must be [{NJOINTS}, 3]")
        self._dev = {}

    @classmethod
    def from_datamodule(cls, dm, **kwargs):
        hp = getattr(dm, "hparams", None)
        mean = getattr(hp, "mean", None) if hp is not None else None
        std = getattr(hp, "std", None) if hp is not None else None
        if mean is None:
            mean, std = getattr(dm, "mean", None), getattr(dm, "std", None)
        if mean is None or std is None or getattr(dm, "njoints", None) != NJOINTS:
            return None
        if len(mean) != NFEATS:
            return None
        return cls(mean, std, NJOINTS, **kwargs)

    def check(self, shape, lengths, normalize=False):
        """The argument checks of a call, without a device: shape [L,22,3] or [B,L,22,3]; returns (B, L, lengths as ints)."""
        if normalize and self.mean is None:
            raise ValueError("normalize=True needs the mean / std statistics")
        shape = tuple(shape)
        if len(shape) not in (3, 4) or shape[-2:] != (NJOINTS, 3):
            raise ValueError(f"joints must be [L, {NJOINTS}, 3] or [B, L, {NJOINTS}, 3], got {shape}")
        B, L = (1, shape[0]) if len(shape) == 3 else shape[:2]
        if not 2 <= L <= MAX_FRAMES:
            raise ValueError(f"joints2feats takes 2 .. {MAX_FRAMES} frames, got {L}")
        if lengths is None:
            lengths = [L] * B
        lengths = [int(l) for l in lengths]
        if len(lengths) != B:
            raise ValueError(f"{len(lengths)} lengths for {B} motions")
        if any(l < 2 or l > L for l in lengths):
            raise ValueError(f"lengths must lie in [2, {L}], got {lengths}")
        return B, L, lengths

    def __call__(self, joints, lengths=None, normalize=False):
        if not torch.is_tensor(joints):
            raise TypeError("joints must be a tensor")
        if not joints.is_cuda:
            raise _lib.LadiffHipError("libladiff_hip works on GPU tensors only; got a CPU tensor (no CPU fallback exists)")
        B, L, lengths = self.check(joints.shape, lengths, normalize)
        dev = joints.device
        if dev not in self._dev:
            self._dev[dev] = tuple(None if t is None else t.to(dev) for t in (self.mean, self.std, self.target_offsets))
        mean, std, tgt = self._dev[dev]
        if not normalize:
            mean = std = None
        x = joints.detach().to(torch.float32).contiguous()
        feats = torch.empty(B, L - 1, NFEATS, dtype=torch.float32, device=dev)
        if B:
            h_len = (_lib.ctypes.c_int32 * B)(*lengths)
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().ladiff_joints2feats(_lib.ptr(x), h_len, B, L, NJOINTS, _lib.ptr(tgt), self.feet_thre, _lib.ptr(mean),
                                                          _lib.ptr(std), _lib.ptr(feats), torch.cuda.current_stream(dev).cuda_stream))
        feats = feats.to(joints.dtype) if joints.dtype.is_floating_point else feats
        return feats[0] if joints.dim() == 3 else feats
