"""numpy float64 restatement of the two joint-space metrics (test infrastructure, like tests/trained_like.py): what
`ladiff_joint_ape_ave` and `ladiff_joint_mr` compute, one row of sums per sequence, and the few divisions of `compute()`.
Written from the description of the metrics (include/ladiff_hip.h), not from the kernels; checked against values recorded from the
reference's own classes (tests/golden/make_golden_joint_metrics.py) in tests/test_joint_metrics.py."""
import numpy as np

# positions of LS, RS, LH, RH, LMrot, RMrot, LF, RF in the reference's joint-name lists
PARTS = {"humanml3d": (17, 16, 2, 1, 8, 7, 11, 10), "mmm": (5, 8, 11, 16, 14, 19, 15, 20)}


def ape_ave_factor(jointstype, force_in_meter=True):
    if not force_in_meter:
        return 1.0
    return 1000.0 if jointstype == "mmm" else 1000.0 * 0.75 / 480.0


def _transform(joints, parts, factor):
    """[F,J,3] -> global joints [F,J,3], local poses [F,J-1,3], root [F,3], trajectory [F,2], all divided by `factor`."""
    LS, RS, LH, RH, LM, RM, LF, RF = parts
    x = np.array(joints, dtype=np.float64)
    F = x.shape[0]
    feet = x[:, [LM, LF, RM, RF], 1].min(axis=1)                      # per frame; the soft minimum sees every frame of the tensor
    lo, hi = feet.min(), feet.max()
    x[:, :, 1] -= lo - np.log(0.5 + np.exp(lo - hi))
    root_y = x[:, 0, 1].copy()
    traj = x[:, 0, [0, 2]].copy()
    poses = x[:, 1:, :].copy()                                        # the root joint removed: hips and shoulders index THIS
    poses[:, :, 0] -= traj[:, None, 0]
    poses[:, :, 2] -= traj[:, None, 1]
    vel = np.zeros_like(traj)
    vel[1:] = traj[1:] - traj[:-1]
    across = poses[:, RH] - poses[:, LH] + poses[:, RS] - poses[:, LS]
    fwd = np.stack([-across[:, 2], across[:, 0]], axis=-1)
    fwd = fwd / np.maximum(np.linalg.norm(fwd, axis=-1, keepdims=True), 1e-12)
    angle = np.arctan2(fwd[:, 0], fwd[:, 1])
    vel_angle = np.zeros(F)
    vel_angle[1:] = angle[1:] - angle[:-1]
    s, c = fwd[:, 0], fwd[:, 1]                                       # into the frame's own heading
    local = np.stack([poses[:, :, 0] * c[:, None] - poses[:, :, 2] * s[:, None], poses[:, :, 1],
                      poses[:, :, 0] * s[:, None] + poses[:, :, 2] * c[:, None]], axis=-1)
    vel_local = np.stack([vel[:, 0] * c - vel[:, 1] * s, vel[:, 0] * s + vel[:, 1] * c], axis=-1)
    ang = np.cumsum(vel_angle)
    ang = ang - ang[0]
    c2, s2 = np.cos(ang), np.sin(ang)                                 # back out by the integrated heading
    rot = np.stack([local[:, :, 0] * c2[:, None] + local[:, :, 2] * s2[:, None], local[:, :, 1],
                    -local[:, :, 0] * s2[:, None] + local[:, :, 2] * c2[:, None]], axis=-1)
    vel_world = np.stack([vel_local[:, 0] * c2 + vel_local[:, 1] * s2, -vel_local[:, 0] * s2 + vel_local[:, 1] * c2], axis=-1)
    trajectory = np.cumsum(vel_world, axis=0)
    trajectory = trajectory - trajectory[0]
    root = np.stack([trajectory[:, 0], root_y, trajectory[:, 1]], axis=-1)
    glob = np.concatenate([np.zeros((F, 1, 3)), rot], axis=1)
    glob[:, 0, 1] = root_y
    glob[:, :, 0] += trajectory[:, None, 0]
    glob[:, :, 2] += trajectory[:, None, 1]
    return glob / factor, local / factor, root / factor, trajectory / factor


def _var(x, T):
    return ((x - x.mean(axis=0)) ** 2).sum(axis=0) / (T - 1)


def ape_ave_rows(rst, ref, lengths, jointstype="humanml3d", force_in_meter=True):
    """[B, W] float64, W = 4 + 2 (J - 1) + 2 J: APE_root, APE_traj, APE_pose[J-1], APE_joints[J], AVE_root, AVE_traj, AVE_pose[J-1],
    AVE_joints[J] of each sequence."""
    parts, factor = PARTS[jointstype], ape_ave_factor(jointstype, force_in_meter)
    rows = []
    for a, b, n in zip(np.asarray(rst), np.asarray(ref), lengths):
        n = int(n)
        ta = [v[:n] for v in _transform(a, parts, factor)]
        tb = [v[:n] for v in _transform(b, parts, factor)]
        ape = [np.linalg.norm(p - q, axis=-1).sum(axis=0) for p, q in zip(ta, tb)]          # joints, pose, root, traj
        with np.errstate(divide="ignore", invalid="ignore"):
            ave = [np.linalg.norm(_var(p, n) - _var(q, n), axis=-1) for p, q in zip(ta, tb)]
        rows.append(np.concatenate([np.atleast_1d(v) for v in (ape[2], ape[3], ape[1], ape[0], ave[2], ave[3], ave[1], ave[0])]))
    return np.stack(rows)


def _similarity(S1, S2):
    """[D,N] point sets: S1 moved onto S2 by the best scale, rotation and translation."""
    mu1, mu2 = S1.mean(axis=1, keepdims=True), S2.mean(axis=1, keepdims=True)
    x1, x2 = S1 - mu1, S2 - mu2
    K = x1 @ x2.T
    U, _, Vt = np.linalg.svd(K)
    Z = np.eye(K.shape[0])
    Z[-1, -1] = np.sign(np.linalg.det(U @ Vt))
    R = Vt.T @ Z @ U.T
    scale = np.trace(R @ K) / (x1 ** 2).sum()
    return scale * (R @ S1) + (mu2 - scale * (R @ mu1))


def mr_rows(rst, ref):
    """[B, 3] float64: the sums over ALL frames of each sequence of the per-frame MPJPE, PA-MPJPE and ACCEL."""
    rows = []
    for a, b in zip(np.asarray(rst, dtype=np.float64), np.asarray(ref, dtype=np.float64)):
        F, J = a.shape[:2]
        mask = (b[:, :, 0] != -2.0).astype(np.float64)
        d = np.linalg.norm((a - a[:, :1]) - (b - b[:, :1]), axis=-1)
        mpjpe = ((d * mask).sum(axis=1) / mask.sum(axis=1)).sum()
        # the reference transposes a [F,J,3] tensor to [F,3,J] only when F is neither 3 nor 2 (utils.py:274-278): a 3- or 2-frame tensor
        # is taken as transposed already, and each frame is then aligned as 3 points in J dimensions (the means run over x, y, z)
        as_points = (lambda m: m) if F in (2, 3) else (lambda m: m.T)
        pa = sum(np.linalg.norm(as_points(_similarity(as_points(s1), as_points(s2))) - s2, axis=-1).mean() for s1, s2 in zip(a, b))
        accel = 0.0
        if F >= 3:
            acc_a = a[:-2] - 2 * a[1:-1] + a[2:]
            acc_b = b[:-2] - 2 * b[1:-1] + b[2:]
            accel = np.linalg.norm(acc_a - acc_b, axis=-1).mean(axis=1).sum()
        rows.append([mpjpe, pa, accel])
    return np.array(rows, dtype=np.float64)


def ape_ave_compute(sums, count, count_seq, njoints):
    J = njoints
    s = np.asarray(sums, dtype=np.float64)
    ape, ave = s[:2 * J + 1], s[2 * J + 1:]
    out = {}
    for tag, part, div in (("APE", ape, count), ("AVE", ave, count_seq)):
        out[f"{tag}_root"] = part[0] / div
        out[f"{tag}_traj"] = part[1] / div
        out[f"{tag}_mean_pose"] = part[2:2 + J - 1].mean() / div
        out[f"{tag}_mean_joints"] = part[2 + J - 1:].mean() / div
    return out


def mr_compute(sums, count, count_seq, force_in_meter=True):
    f = 1000.0 if force_in_meter else 1.0
    s = np.asarray(sums, dtype=np.float64)
    return {"MPJPE": s[0] / count * f, "PAMPJPE": s[1] / count * f, "ACCEL": s[2] / (count - 2 * count_seq) * f}
