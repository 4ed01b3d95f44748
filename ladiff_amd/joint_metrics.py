"""The reference's joint-space metric classes on the GPU: `ComputeMetrics` (= "TemosMetric": APE / AVE, models/metrics/compute.py) and
`MRMetrics` (MPJPE / PA-MPJPE / ACCEL, models/metrics/mr.py), fed with the `joints_rst` / `joints_ref` [B,F,J,3] that `t2m_eval` returns
(ladiff.py:1443-1445, :1464-1466).  `update()` queues two launches (`ladiff_joint_ape_ave` / `ladiff_joint_mr`: one row of sums per
sequence, then the rows added to an fp64 accumulator in sequence order) and returns without synchronising; `compute()` copies the
accumulator once and does the reference's few divisions in numpy.  There is no CPU implementation.
"""
import ctypes

import numpy as np
import torch

from . import _lib

# positions of LS, RS, LH, RH, LMrot, RMrot, LF, RF in the reference's joint-name lists (utils/joints.py:1-48); KIT's 21-joint tensors
# are configured with the humanml3d list too (config_ladiff_kit.yaml:94)
PART_INDEX = {"humanml3d": (17, 16, 2, 1, 8, 7, 11, 10), "mmm": (5, 8, 11, 16, 14, 19, 15, 20)}


class _JointMetric:
    """State shared by the two classes: `count`, `count_seq` (host ints) and the fp64 sums (on the device while updates are queued)."""
    _width = 0

    def __init__(self, njoints, jointstype="mmm", force_in_meter=True, dist_sync_on_step=True, **kwargs):
        if jointstype not in PART_INDEX:
            raise NotImplementedError("This jointstype is not implemented.")
        self.njoints, self.jointstype, self.force_in_meter = int(njoints), jointstype, force_in_meter
        self.reset()

    def reset(self):
        self.count, self.count_seq = 0, 0
        self._host = np.zeros(self._width, dtype=np.float64)   # sums merged in by add_sums / folded from another device
        self._acc = None                                       # fp64 [W] on the device the updates run on
        self.last_rows = None                                  # [B, W] fp32 device tensor of the latest update: its per-sequence sums

    def _launch(self, L, rst, ref, d_lengths, h_lengths, B, F, J, rows, stream):
        raise NotImplementedError

    def update(self, joints_rst, joints_ref, lengths):
        if joints_rst.dim() != 4 or tuple(joints_rst.shape) != tuple(joints_ref.shape) or joints_rst.shape[-1] != 3:
            raise _lib.LadiffHipError(f"joint metrics take two [B,F,J,3] tensors, got {tuple(joints_rst.shape)} and {tuple(joints_ref.shape)}")
        lengths = [int(l) for l in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
        B, F, J, _ = joints_rst.shape
        if len(lengths) != B:
            raise _lib.LadiffHipError(f"{len(lengths)} lengths for {B} sequences")
        if J != self.njoints:
            raise _lib.LadiffHipError(f"built for {self.njoints} joints, got {J}")
        if B == 0:
            return
        device = next((t.device for t in (joints_rst, joints_ref) if t.is_cuda), None)
        if device is None:
            if not torch.cuda.is_available():
                raise _lib.LadiffHipError("joint metrics run on the GPU only; got CPU tensors and there is no GPU (no CPU fallback exists)")
            device = torch.device("cuda", torch.cuda.current_device())
        L = _lib.lib()
        with torch.cuda.device(device):
            rst = joints_rst.detach().to(device=device, dtype=torch.float32).contiguous()
            ref = joints_ref.detach().to(device=device, dtype=torch.float32).contiguous()
            if self._acc is not None and self._acc.device != device:
                self._host += self._acc.cpu().numpy()
                self._acc = None
            if self._acc is None:
                self._acc = torch.zeros(self._width, dtype=torch.float64, device=device)
            rows = torch.empty(B, self._width, dtype=torch.float32, device=device)
            h_lengths = (ctypes.c_int32 * B)(*lengths)
            _lib.check(self._launch(L, rst, ref, _lib.device_ints(lengths, device), h_lengths, B, F, J, rows,
                                    torch.cuda.current_stream(device).cuda_stream))
        self.last_rows = rows
        self.count += sum(lengths)
        self.count_seq += B

    def sums(self):
        """{"count", "count_seq", "sums"}: the two counts and the fp64 sums [W] as a numpy array (waits for the queued updates)."""
        total = self._host.copy()
        if self._acc is not None:
            total += self._acc.cpu().numpy()
        return {"count": self.count, "count_seq": self.count_seq, "sums": total}

    def add_sums(self, other):
        """Merge another object's state (its `sums()` dict, or the object): the reference's dist_reduce_fx="sum"."""
        other = other.sums() if hasattr(other, "sums") else other
        add = np.asarray(other["sums"], dtype=np.float64)
        if add.shape != self._host.shape:
            raise ValueError(f"sums of {add.shape[0]} values merged into {self._host.shape[0]}")
        self._host += add
        self.count += int(other["count"])
        self.count_seq += int(other["count_seq"])


class ComputeMetrics(_JointMetric):
    """APE and AVE of root, trajectory, local poses and global joints (compute.py:15-196).  Sums layout [W = 4 + 2 (J-1) + 2 J]:
    APE_root, APE_traj, APE_pose[J-1], APE_joints[J], AVE_root, AVE_traj, AVE_pose[J-1], AVE_joints[J]."""

    def __init__(self, njoints, jointstype="mmm", force_in_meter=True, dist_sync_on_step=True, **kwargs):
        self.name = "APE and AVE"
        self.APE_metrics = ["APE_root", "APE_traj", "APE_pose", "APE_joints"]
        self.AVE_metrics = ["AVE_root", "AVE_traj", "AVE_pose", "AVE_joints"]
        self.metrics = self.APE_metrics + self.AVE_metrics
        self._width = 4 + 2 * (int(njoints) - 1) + 2 * int(njoints)
        super().__init__(njoints, jointstype, force_in_meter, dist_sync_on_step, **kwargs)
        self.factor = (1000.0 if jointstype == "mmm" else 1000.0 * 0.75 / 480.0) if force_in_meter else 1.0      # compute.py:181-186
        self._parts = (ctypes.c_int32 * 8)(*PART_INDEX[jointstype])

    def _launch(self, L, rst, ref, d_lengths, h_lengths, B, F, J, rows, stream):
        return L.ladiff_joint_ape_ave(rst.data_ptr(), ref.data_ptr(), d_lengths.data_ptr(), ctypes.cast(h_lengths, ctypes.c_void_p), B, F, J,
                                      ctypes.cast(self._parts, ctypes.c_void_p), self.factor, rows.data_ptr(), self._acc.data_ptr(), stream)

    def compute(self, sanity_flag=False):
        """The reference's keys and divisors (compute.py:71-100): APE over `count` frames, AVE over `count_seq` sequences."""
        st, J = self.sums(), self.njoints
        s = st["sums"]
        out = {}
        with np.errstate(divide="ignore", invalid="ignore"):
            for tag, part, div in (("APE", s[:2 * J + 1], st["count"]), ("AVE", s[2 * J + 1:], st["count_seq"])):
                div = np.float64(div)
                out[f"{tag}_root"] = float(part[0] / div)
                out[f"{tag}_traj"] = float(part[1] / div)
                out[f"{tag}_mean_pose"] = float(part[2:2 + J - 1].mean() / div)
                out[f"{tag}_mean_joints"] = float(part[2 + J - 1:].mean() / div)
        return out


TemosMetric = ComputeMetrics


class MRMetrics(_JointMetric):
    """Motion-reconstruction metrics (mr.py:11-96).  Sums layout [3]: MPJPE, PAMPJPE, ACCEL, each summed over EVERY frame of the padded
    sequences, as the reference does."""
    _width = 3

    def __init__(self, njoints, jointstype="mmm", force_in_meter=True, align_root=True, dist_sync_on_step=True, **kwargs):
        if not align_root:
            raise NotImplementedError("MRMetrics(align_root=False) is not built: MPJPE is root-aligned")
        self.name = "Motion Reconstructions"
        self.align_root = align_root
        self.MR_metrics = ["MPJPE", "PAMPJPE", "ACCEL"]
        self.metrics = self.MR_metrics
        super().__init__(njoints, jointstype, force_in_meter, dist_sync_on_step, **kwargs)

    def _launch(self, L, rst, ref, d_lengths, h_lengths, B, F, J, rows, stream):
        return L.ladiff_joint_mr(rst.data_ptr(), ref.data_ptr(), ctypes.cast(h_lengths, ctypes.c_void_p), B, F, J, rows.data_ptr(),
                                 self._acc.data_ptr(), stream)

    def compute(self, sanity_flag=False):
        """mr.py:52-71: per frame over `count`, ACCEL over `count - 2 * count_seq`, times 1000 when force_in_meter."""
        st = self.sums()
        s, factor = st["sums"], (1000.0 if self.force_in_meter else 1.0)
        count, count_seq = np.float64(st["count"]), np.float64(st["count_seq"])
        with np.errstate(divide="ignore", invalid="ignore"):
            return {"MPJPE": float(s[0] / count * factor), "PAMPJPE": float(s[1] / count * factor),
                    "ACCEL": float(s[2] / (count - 2 * count_seq) * factor)}
