"""numpy restatement of the reference's joints -> HumanML3D features path: `process_file` (data/humanml/scripts/motion_process.py:169-351),
`uniform_skeleton` (:13-36), `Skeleton.inverse_kinematics_np / forward_kinematics_np / get_offsets_joints` (common/skeleton.py:43-147),
the quaternion helpers (common/quaternion.py) and scipy's `gaussian_filter1d(., 20, mode='nearest')`.  TEST INFRASTRUCTURE ONLY (a plain
helper module, like joint_metrics_ref.py): what `ladiff_joints2feats` is held against, itself pinned to values recorded from the
reference (tests/golden/make_golden_joints2feats.py) in tests/test_joints2feats.py.  No reference import, no scipy.

The reference mixes number formats, and the restatement follows it op for op: every quaternion helper with an `_np` suffix converts its
arguments to float32, works in float32 and returns float32 (`torch.from_numpy(q).float()`), the skeleton's offsets are float32, and
`qrot_np` turns the positions themselves into float32 at motion_process.py:213 - everything after the initial facing is float32 but
the forward vector's cross product, its smoothing and its normalisation.  `dtype=np.float32` runs those remaining float64 steps in
float32 as well: the format of the kernel."""
import numpy as np

F32 = np.float32

# the t2m skeleton (utils/paramUtil.py): five chains walked in this order, each starting from the ROOT's rotation
CHAINS = [[0, 2, 5, 8, 11], [0, 1, 4, 7, 10], [0, 3, 6, 9, 12, 15], [9, 14, 17, 19, 21], [9, 13, 16, 18, 20]]
RAW_OFFSETS = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, -1, 0], [0, 1, 0], [0, -1, 0], [0, -1, 0], [0, 1, 0],
                        [0, 0, 1], [0, 0, 1], [0, 1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, -1, 0], [0, -1, 0], [0, -1, 0], [0, -1, 0],
                        [0, -1, 0], [0, -1, 0]])
PARENTS = [-1] + [0] * 21
for _c in CHAINS:
    for _j in range(1, len(_c)):
        PARENTS[_c[_j]] = _c[_j - 1]
FACE_JOINT_INDX = [2, 1, 17, 16]
FID_R, FID_L = [8, 11], [7, 10]
L_IDX1, L_IDX2 = 5, 8
FEET_THRE = 0.002                    # motion_process.py:468
NFEATS = 263
CONTACT_COLS = slice(259, 263)


# ------------------------------------------------------------------------------------------ quaternion.py, the float32 helpers
def _sum3(a):
    return (a[..., 0] + a[..., 1]) + a[..., 2]


def _cross(a, b, axis=-1):
    """torch.cross on float32, as its CPU kernel rounds it: each component is fma(a1, b2, -(a2 * b1)), the second product rounded first.
    (Both products are exact in float64, so the fused form is one float64 subtraction rounded to float32.)"""
    a, b = np.moveaxis(a, axis, -1), np.moveaxis(b, axis, -1)
    d = np.float64

    def comp(p, q, r, s):
        return (p.astype(d) * q.astype(d) - (r * s).astype(d)).astype(F32)

    out = np.stack([comp(a[..., 1], b[..., 2], a[..., 2], b[..., 1]), comp(a[..., 2], b[..., 0], a[..., 0], b[..., 2]),
                    comp(a[..., 0], b[..., 1], a[..., 1], b[..., 0])], axis=-1)
    return np.moveaxis(out, -1, axis)


def qinv(q):
    q = np.asarray(q).astype(F32)
    return q * np.array([1, -1, -1, -1], dtype=F32)


def qmul(q, r):
    q, r = np.asarray(q).astype(F32), np.asarray(r).astype(F32)
    t = r[..., :, None] * q[..., None, :]
    w = t[..., 0, 0] - t[..., 1, 1] - t[..., 2, 2] - t[..., 3, 3]
    x = t[..., 0, 1] + t[..., 1, 0] - t[..., 2, 3] + t[..., 3, 2]
    y = t[..., 0, 2] + t[..., 1, 3] + t[..., 2, 0] - t[..., 3, 1]
    z = t[..., 0, 3] - t[..., 1, 2] + t[..., 2, 1] + t[..., 3, 0]
    return np.stack([w, x, y, z], axis=-1)


def qrot(q, v):
    q, v = np.asarray(q).astype(F32), np.asarray(v).astype(F32)
    qvec = q[..., 1:]
    uv = _cross(qvec, v)
    uuv = _cross(qvec, uv)
    return v + F32(2) * (q[..., :1] * uv + uuv)


def qbetween(v0, v1, trace=None):
    """normalize([|v0||v1| + v0.v1, v0 x v1]): no special case for anti-parallel vectors (quaternion.py:387-397).  The reference calls
    `torch.cross(v0, v1)` WITHOUT a dim, which takes the first dimension of size 3: for the [L, 3] arguments of a 3-frame motion that
    is the FRAME axis, not the coordinate axis (every other length, and the [1, 3] call of the initial facing, take the coordinates)."""
    v0, v1 = np.asarray(v0).astype(F32), np.asarray(v1).astype(F32)
    v = _cross(v0, v1, axis=v0.shape.index(3))
    w = np.sqrt(_sum3(v0 ** 2) * _sum3(v1 ** 2)) + _sum3(v0 * v1)
    if trace is not None:
        trace["w"] = min(trace.get("w", np.inf), float(np.min(w)))
    q = np.concatenate([w[..., None], v], axis=-1)
    n = np.sqrt(((q[..., 0] ** 2 + q[..., 1] ** 2) + q[..., 2] ** 2) + q[..., 3] ** 2)
    return q / n[..., None]


def quaternion_to_cont6d(q):
    q = np.asarray(q).astype(F32)
    r, i, j, k = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    two_s = F32(2) / (((q[..., 0] ** 2 + q[..., 1] ** 2) + q[..., 2] ** 2) + q[..., 3] ** 2)
    one = F32(1)
    # columns 0 and 1 of the rotation matrix (quaternion.py:274-311)
    return np.stack([one - two_s * (j * j + k * k), two_s * (i * j + k * r), two_s * (i * k - j * r),
                     two_s * (i * j - k * r), one - two_s * (i * i + k * k), two_s * (j * k + i * r)], axis=-1)


# ------------------------------------------------------------------------------------------ scipy.ndimage.gaussian_filter1d
def gaussian_weights(sigma=20, dtype=np.float64):
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return (phi / phi.sum()).astype(dtype), radius


def gaussian_filter1d_nearest(a, sigma=20):
    """Along axis 0, edge frames replicated; the symmetric form scipy's correlate1d takes for a symmetric kernel."""
    w, radius = gaussian_weights(sigma, a.dtype)
    n = len(a)
    idx = np.arange(n)
    out = a * w[radius]
    for k in range(1, radius + 1):
        out = out + (a[np.clip(idx - k, 0, n - 1)] + a[np.clip(idx + k, 0, n - 1)]) * w[radius + k]
    return out


# ------------------------------------------------------------------------------------------ skeleton.py
def get_offsets_joints(pose):
    """Skeleton.get_offsets_joints: raw direction x bone length of `pose` [22, 3], float32."""
    pose = np.asarray(pose)
    off = RAW_OFFSETS.astype(F32)
    for i in range(1, 22):
        d = pose[i] - pose[PARENTS[i]]
        off[i] = F32(np.sqrt((d ** 2).sum())) * off[i]
    return off


def inverse_kinematics(joints, smooth_forward, dtype=np.float64, trace=None):
    """Skeleton.inverse_kinematics_np: note the unpacking - the list that process_file reads as r_hip, l_hip, sdr_r, sdr_l is read
    here as l_hip, r_hip, sdr_r, sdr_l, so the hip term enters `across` with the opposite sign (skeleton.py:58-61)."""
    l_hip, r_hip, sdr_r, sdr_l = FACE_JOINT_INDX
    across = (joints[:, r_hip] - joints[:, l_hip]) + (joints[:, sdr_r] - joints[:, sdr_l])
    across = across / np.sqrt((across ** 2).sum(axis=-1))[:, None]
    # np.cross([[0, 1, 0]], across): an int64 operand, so float32 positions give a float64 forward vector in the reference (= dtype)
    forward = np.stack([across[:, 2], np.zeros_like(across[:, 0]), -across[:, 0]], axis=-1).astype(dtype)
    if smooth_forward:
        forward = gaussian_filter1d_nearest(forward, 20)
    forward = forward / np.sqrt((forward ** 2).sum(axis=-1))[:, None]
    target = np.zeros_like(forward)
    target[:, 2] = 1
    root_quat = qbetween(forward, target, trace)
    root_quat[0] = np.array([1, 0, 0, 0], dtype=F32)
    quat = np.zeros(joints.shape[:-1] + (4,), dtype=F32)          # float64 in the reference, holding float32 values
    quat[:, 0] = root_quat
    for chain in CHAINS:
        R = root_quat
        for j in range(len(chain) - 1):
            u = np.repeat(RAW_OFFSETS[chain[j + 1]][None], len(joints), axis=0)
            v = joints[:, chain[j + 1]] - joints[:, chain[j]]
            v = v / np.sqrt((v ** 2).sum(axis=-1))[:, None]
            rot_u_v = qbetween(u, v, trace)
            R_loc = qmul(qinv(R), rot_u_v)
            quat[:, chain[j + 1]] = R_loc
            R = qmul(R, R_loc)
    return quat


def forward_kinematics(quat, root_pos, offsets):
    joints = np.zeros(quat.shape[:-1] + (3,), dtype=root_pos.dtype)
    joints[:, 0] = root_pos
    for chain in CHAINS:
        R = quat[:, 0]
        for i in range(1, len(chain)):
            R = qmul(R, quat[:, chain[i]])
            off = np.repeat(offsets[chain[i]][None], len(quat), axis=0)
            joints[:, chain[i]] = qrot(R, off) + joints[:, chain[i - 1]]
    return joints


def uniform_skeleton(positions, tgt_offsets, trace=None):
    tgt = np.asarray(tgt_offsets).astype(F32)
    src = get_offsets_joints(positions[0])
    src_leg = np.abs(src[L_IDX1]).max() + np.abs(src[L_IDX2]).max()
    tgt_leg = np.abs(tgt[L_IDX1]).max() + np.abs(tgt[L_IDX2]).max()
    scale_rt = F32(tgt_leg / src_leg)
    root = positions[:, 0] * positions.dtype.type(scale_rt)
    quat = inverse_kinematics(positions, False, positions.dtype.type, trace)
    return forward_kinematics(quat, root, tgt)


# ------------------------------------------------------------------------------------------ motion_process.py:169-351
def process_file(positions, feet_thre=FEET_THRE, tgt_offsets=None, dtype=np.float64, trace=None):
    """features [L - 1, 263] of positions [L, 22, 3].  tgt_offsets None: the uniform-skeleton step is the identity.  dtype: the format of
    the steps the reference runs in float64 (its input's format); the result is float64 in both modes.  trace (a dict) collects the
    smallest un-normalised w of all qbetween calls ("w") and the feet's squared displacements ("feet", [L - 1, 4])."""
    positions = np.array(positions, dtype=dtype)
    if tgt_offsets is not None:
        positions = uniform_skeleton(positions, tgt_offsets, trace)
    floor = positions.min(axis=0).min(axis=0)[1]
    positions[:, :, 1] -= floor
    root_pos_init = positions[0]
    positions = positions - root_pos_init[0] * np.array([1, 0, 1], dtype=dtype)
    r_hip, l_hip, sdr_r, sdr_l = FACE_JOINT_INDX
    across = (root_pos_init[r_hip] - root_pos_init[l_hip]) + (root_pos_init[sdr_r] - root_pos_init[sdr_l])
    across = across / np.sqrt((across ** 2).sum())
    forward_init = np.array([across[2], 0 * across[0], -across[0]])
    forward_init = forward_init / np.sqrt((forward_init ** 2).sum())
    root_quat_init = qbetween(forward_init[None], np.array([[0, 0, 1]]), trace)
    positions = qrot(np.broadcast_to(root_quat_init, positions.shape[:-1] + (4,)), positions)      # float32 from here on
    global_positions = positions.copy()

    def feet(fid):
        d = positions[1:, fid] - positions[:-1, fid]
        return (d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2

    d_l, d_r = feet(FID_L), feet(FID_R)
    if trace is not None:
        trace["feet"] = np.concatenate([d_l, d_r], axis=-1).astype(np.float64)
    feet_l, feet_r = (d_l < np.float64(feet_thre)).astype(np.float64), (d_r < np.float64(feet_thre)).astype(np.float64)

    quat = inverse_kinematics(positions, True, dtype, trace)
    cont6d = quaternion_to_cont6d(quat)
    r_rot = quat[:, 0].copy()
    velocity = qrot(r_rot[1:], positions[1:, 0] - positions[:-1, 0])
    r_velocity = qmul(r_rot[1:], qinv(r_rot[:-1]))
    # get_rifke
    local = positions.copy()
    local[..., 0] -= positions[:, 0:1, 0]
    local[..., 2] -= positions[:, 0:1, 2]
    local = qrot(np.repeat(r_rot[:, None], 22, axis=1), local)
    root_y = local[:, 0, 1:2]
    r_vel = np.arcsin(r_velocity[:, 2:3])
    l_vel = velocity[:, [0, 2]]
    local_vel = qrot(np.repeat(r_rot[:-1, None], 22, axis=1), global_positions[1:] - global_positions[:-1])
    n = len(positions)
    return np.concatenate([r_vel, l_vel, root_y[:-1], local[:-1, 1:].reshape(n - 1, -1), cont6d[:-1, 1:].reshape(n - 1, -1),
                           local_vel.reshape(n - 1, -1), feet_l, feet_r], axis=-1).astype(np.float64)


# ------------------------------------------------------------------------------------------ test motions
def _roty(v, a):
    c, s = np.cos(a), np.sin(a)
    return np.stack([v[..., 0] * c + v[..., 2] * s, v[..., 1], -v[..., 0] * s + v[..., 2] * c], axis=-1)


def motion(L, seed):
    """A deterministic walking figure on the t2m chains, [L, 22, 3] float64, y up, 20 frames per second.  Human-like proportions
    (shoulder span 0.38 +- 5 %, hip span 0.14 +- 5 %: the inverse kinematics' forward vector is their DIFFERENCE, see
    inverse_kinematics), start heading within +-0.4 rad of +Z, a slow turn, legs and arms swinging in opposition, a torso twist."""
    rng = np.random.default_rng(1000 + seed)
    s = 1.0 + 0.05 * rng.uniform(-1, 1, 8)                                  # proportions
    hip_w, hip_d, thigh, shin = 0.07 * s[0], 0.08 * s[1], 0.40 * s[2], 0.40 * s[3]
    sdr_w, upper, fore, spine = 0.19 * s[4], 0.26 * s[5], 0.25 * s[6], s[7]
    freq = rng.uniform(0.8, 1.1) * 2 * np.pi / 20                           # gait phase per frame
    amp, knee, arm = rng.uniform(0.25, 0.4), rng.uniform(0.3, 0.6), rng.uniform(0.2, 0.5)
    speed = rng.uniform(0.025, 0.05)                                        # metres per frame
    head0, turn = rng.uniform(-0.4, 0.4), rng.uniform(-0.004, 0.004)
    ph0 = rng.uniform(0, 2 * np.pi)
    t = np.arange(L, dtype=np.float64)
    ph = ph0 + freq * t
    heading = head0 + turn * t
    twist = 0.08 * np.sin(ph)

    def down(angle):                                                        # a unit bone hanging down, pitched forward by `angle`
        return np.stack([np.zeros_like(angle), -np.cos(angle), np.sin(angle)], axis=-1)

    P = np.zeros((L, 22, 3))
    z3 = np.zeros(L)
    const = lambda x, y, z: np.stack([z3 + x, z3 + y, z3 + z], axis=-1)
    P[:, 1], P[:, 2] = const(hip_w, -hip_d, 0), const(-hip_w, -hip_d, 0)
    for side, hip, kn, an, ft in ((1, 1, 4, 7, 10), (-1, 2, 5, 8, 11)):
        a = side * amp * np.sin(ph)
        k = knee * 0.5 * (1 + np.sin(ph * side + 0.7))
        P[:, kn] = P[:, hip] + thigh * down(a)
        P[:, an] = P[:, kn] + shin * down(a - k)
        P[:, ft] = P[:, an] + const(0, -0.05, 0.12)
    P[:, 3] = const(0, 0.11 * spine, -0.01)
    P[:, 6] = P[:, 3] + const(0, 0.13 * spine, 0.01)
    P[:, 9] = P[:, 6] + const(0, 0.06 * spine, 0)
    P[:, 12] = P[:, 9] + const(0, 0.20 * spine, 0)
    P[:, 15] = P[:, 12] + const(0, 0.09, 0.03)
    for side, col, sd, el, wr in ((1, 13, 16, 18, 20), (-1, 14, 17, 19, 21)):
        P[:, col] = P[:, 9] + _roty(const(side * 0.08, 0.11 * spine, 0), twist)
        P[:, sd] = P[:, 9] + _roty(const(side * sdr_w, 0.13 * spine, 0), twist)
        a = -side * arm * np.sin(ph)
        P[:, el] = P[:, sd] + upper * down(a)
        P[:, wr] = P[:, el] + fore * down(a + 0.3)
    P = _roty(P, heading[:, None])
    step = speed * np.stack([np.sin(heading), z3, np.cos(heading)], axis=-1)
    root = np.cumsum(step, axis=0) - step[0]
    root[:, 1] = 0.93 * s[2] + 0.02 * np.sin(2 * ph)
    root += np.array([rng.uniform(-1, 1), 0.0, rng.uniform(-1, 1)])
    return P + root[:, None]


def target_pose(seed=0):
    """A standing pose of other proportions: the `example_id` pose the reference's script takes its target offsets from."""
    rng = np.random.default_rng(77 + seed)
    pose = motion(1, 500 + seed)[0]
    pose = pose - pose[0]
    return pose * rng.uniform(0.9, 1.1)


def conditioning(positions, feet_thre=FEET_THRE, tgt_offsets=None):
    """(w, foot margin, s32) of one case: the smallest un-normalised w over all qbetween calls, the smallest relative distance of a
    foot displacement^2 from feet_thre, and the largest change of a non-contact output column when the input is rounded to float32."""
    trace = {}
    want = process_file(positions, feet_thre, tgt_offsets, trace=trace)
    margin = float(np.min(np.abs(trace["feet"] - feet_thre)) / feet_thre)
    rounded = process_file(np.asarray(positions).astype(F32).astype(np.float64), feet_thre, tgt_offsets)
    s32 = float(np.abs(want[:, :259] - rounded[:, :259]).max())
    return trace["w"], margin, s32


# seeds per length for which every case condition holds with and without target offsets (tests/test_joints2feats.py asserts them)
CASE_SEEDS = {2: 1, 3: 1, 40: 1, 82: 1, 162: 1, 197: 1, 256: 1}
W_MIN, MARGIN_MIN, S32_MAX = 0.5, 1e-3, 5e-5


def case(L, with_target):
    """(positions float64 [L,22,3], target offsets float32 [22,3] or None) of the test case at length L."""
    return motion(L, CASE_SEEDS[L]), (get_offsets_joints(target_pose()) if with_target else None)
