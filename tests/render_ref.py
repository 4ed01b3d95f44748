"""numpy restatement of the renderer's image model, written from the text of include/ladiff_hip.h ("motion renderer") and from nothing
else: scene bounds, pinhole camera, ground by ray, bones as capsules with a one-pixel linear edge, compositing in a fixed order.
`dtype=np.float64` is the yardstick; `dtype=np.float32` runs the same statements in single precision (every constant is cast), which is
what the GPU tests take their gate from."""
import numpy as np

# utils/paramUtil.py: t2m_kinematic_chain / kit_kinematic_chain (data, restated)
CHAINS = {22: ((0, 2, 5, 8, 11), (0, 1, 4, 7, 10), (0, 3, 6, 9, 12, 15), (9, 14, 17, 19, 21), (9, 13, 16, 18, 20)),
          21: ((0, 11, 12, 13, 14, 15), (0, 16, 17, 18, 19, 20), (0, 1, 2, 3, 4), (3, 5, 6, 7), (3, 8, 9, 10))}
CHAIN_RGB = tuple(tuple(int(h[i:i + 2], 16) / 255.0 for i in (1, 3, 5)) for h in ("#DD5A37", "#D69E00", "#B75A39", "#DD5A37", "#D69E00"))
TINY = 1e-12


def style(H, **kw):
    """The header's defaults (line_width = H / 54) with `kw` on top."""
    s = dict(elev_deg=15.0, azim_deg=25.0, dist=3.6, focal=2.0, target_height=0.9, near=0.1, line_width=H / 54.0, ground_margin=0.5,
             alpha_min=0.25, strip_fit=3.0, ground_alpha=0.5, background=(1.0, 1.0, 1.0), ground=(0.5, 0.5, 0.5), chain_colors=CHAIN_RGB)
    unknown = set(kw) - set(s)
    assert not unknown, unknown
    s.update(kw)
    return s


def bones(J):
    """(joint, joint, chain) in compositing order: chains in table order, bones in chain order."""
    return [(c[i], c[i + 1], k) for k, c in enumerate(CHAINS[J]) for i in range(len(c) - 1)]


def strip_indices(length, n_poses):
    n = min(int(n_poses), int(length))
    if n == 1:
        return [0]
    return [(k * (length - 1) + (n - 1) // 2) // (n - 1) for k in range(n)]


def scene(joints, length):
    valid = joints[:length].reshape(-1, 3)
    return valid.min(axis=0), valid.max(axis=0)


def camera(st, H, W, dist, dt):
    """E, f, r, u, F of the look-at camera at distance `dist`, in dtype `dt`."""
    rad = dt(np.pi) / dt(180.0)
    el, az = dt(st["elev_deg"]) * rad, dt(st["azim_deg"]) * rad
    T = np.array([0.0, st["target_height"], 0.0], dtype=dt)
    E = T + dt(dist) * np.array([np.cos(el) * np.sin(az), np.sin(el), np.cos(el) * np.cos(az)], dtype=dt)
    f = T - E
    f = f / np.sqrt((f * f).sum(dtype=dt))
    r = np.cross(f, np.array([0.0, 1.0, 0.0], dtype=dt))
    r = r / np.sqrt((r * r).sum(dtype=dt))
    u = np.cross(r, f)
    return dict(E=E, f=f, r=r, u=u, F=dt(st["focal"]) * dt(H) / dt(2.0), H=H, W=W)


def project(P, cam, dt):
    """Points [N,3] -> (sx, sy, zc)."""
    d = P - cam["E"]
    zc = d @ cam["f"]
    sx = dt(cam["W"]) / dt(2.0) + cam["F"] * (d @ cam["r"]) / zc
    sy = dt(cam["H"]) / dt(2.0) - cam["F"] * (d @ cam["u"]) / zc
    return sx, sy, zc


def pixel_centres(H, W, dt):
    px = (np.arange(W, dtype=dt) + dt(0.5))[None, :]
    py = (np.arange(H, dtype=dt) + dt(0.5))[:, None]
    return px, py


def clamp01(v, dt):
    return np.minimum(np.maximum(v, dt(0.0)), dt(1.0))


def ground_coverage(cam, rect, dt):
    x0, x1, z0, z1 = rect
    px, py = pixel_centres(cam["H"], cam["W"], dt)
    cx = (px - dt(cam["W"]) / dt(2.0)) / cam["F"]
    cy = -(py - dt(cam["H"]) / dt(2.0)) / cam["F"]
    f, r, u, E = cam["f"], cam["r"], cam["u"], cam["E"]
    D = [f[k] + cx * r[k] + cy * u[k] for k in range(3)]
    down = D[1] < 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        th = -E[1] / np.where(down, D[1], dt(-1.0))
        hx, hz = E[0] + th * D[0], E[2] + th * D[2]
        sd = np.minimum(np.minimum(hx - x0, x1 - hx), np.minimum(hz - z0, z1 - hz))
        cov = clamp01(dt(0.5) + sd * cam["F"] / th, dt)
    return np.where(down, cov, dt(0.0)).astype(dt)


def bone_coverage(A, B, H, W, width, dt):
    px, py = pixel_centres(H, W, dt)
    ex, ey = B[0] - A[0], B[1] - A[1]
    s = clamp01(((px - A[0]) * ex + (py - A[1]) * ey) / np.maximum(ex * ex + ey * ey, dt(TINY)), dt)
    qx, qy = px - (A[0] + s * ex), py - (A[1] + s * ey)
    dist2d = np.sqrt(qx * qx + qy * qy)
    return clamp01(dt(0.5) + dt(width) / dt(2.0) - dist2d, dt)


def over(c, q, colour, dt):
    """c <- c (1 - q) + colour q, per channel; q [H,W]."""
    q = q[..., None]
    return c * (dt(1.0) - q) + np.asarray(colour, dtype=dt) * q


def image(poses, rect, cam, st, J, dt):
    """poses: [(points [J,3] in the camera's world, opacity)] in time order."""
    H, W = cam["H"], cam["W"]
    c = np.empty((H, W, 3), dtype=dt)
    c[:] = np.asarray(st["background"], dtype=dt)
    c = over(c, dt(st["ground_alpha"]) * ground_coverage(cam, rect, dt), st["ground"], dt)
    for P, a in poses:
        sx, sy, zc = project(P, cam, dt)
        for ja, jb, chain in bones(J):
            if not (zc[ja] > dt(st["near"]) and zc[jb] > dt(st["near"])):
                continue
            cov = bone_coverage((sx[ja], sy[ja]), (sx[jb], sy[jb]), H, W, st["line_width"], dt)
            c = over(c, dt(a) * cov, st["chain_colors"][chain], dt)
    return c


def render_frames(joints, length, H, W, st=None, dtype=np.float64, frame_stride=1):
    """joints [L,J,3] -> [ceil(L / frame_stride), H, W, 3]; images of frames >= length are background."""
    dt = np.dtype(dtype).type
    st = st or style(H)
    x = np.asarray(joints).astype(dt)
    L, J = x.shape[:2]
    mins, maxs = scene(x, length)
    cam = camera(st, H, W, st["dist"], dt)
    out = []
    for t in range(0, L, frame_stride):
        if t >= length:
            bg = np.empty((H, W, 3), dtype=dt)
            bg[:] = np.asarray(st["background"], dtype=dt)
            out.append(bg)
            continue
        rx, rz = x[t, 0, 0], x[t, 0, 2]
        P = x[t] - np.array([rx, mins[1], rz], dtype=dt)
        rect = (mins[0] - rx, maxs[0] - rx, mins[2] - rz, maxs[2] - rz)
        out.append(image([(P, 1.0)], rect, cam, st, J, dt))
    return np.stack(out)


def strip_distance(st, mins, maxs, dt):
    extent = np.maximum(maxs[0] - mins[0], maxs[2] - mins[2])
    return dt(st["dist"]) * np.maximum(dt(1.0), extent / dt(st["strip_fit"]))


def render_strip(joints, length, n_poses, H, W, st=None, dtype=np.float64):
    """joints [L,J,3] -> [H, W, 3]."""
    dt = np.dtype(dtype).type
    st = st or style(H)
    x = np.asarray(joints).astype(dt)
    J = x.shape[1]
    mins, maxs = scene(x, length)
    cam = camera(st, H, W, strip_distance(st, mins, maxs, dt), dt)
    cx, cz = (mins[0] + maxs[0]) / dt(2.0), (mins[2] + maxs[2]) / dt(2.0)
    m = dt(st["ground_margin"])
    rect = (mins[0] - cx - m, maxs[0] - cx + m, mins[2] - cz - m, maxs[2] - cz + m)
    idx = strip_indices(length, n_poses)
    n = len(idx)
    poses = []
    for k, t in enumerate(idx):
        a = dt(1.0) if n == 1 else dt(st["alpha_min"]) + (dt(1.0) - dt(st["alpha_min"])) * (dt(k) / dt(n - 1))
        poses.append((x[t] - np.array([cx, mins[1], cz], dtype=dt), a))
    return image(poses, rect, cam, st, J, dt)


def to_uint8(img):
    return np.floor(255.0 * np.asarray(img, dtype=np.float64) + 0.5).astype(np.uint8)


# ---- synthetic motions for the tests: a standing figure whose joints hang on the skeleton's chains, walking and swaying
def standing_pose(J=22):
    """[J,3] float64: a plausible upright figure about 1.7 tall, facing +z, root at (0, 0.95, 0)."""
    p = np.zeros((J, 3))
    if J == 22:
        legs, spine, arms = (CHAINS[22][0], CHAINS[22][1]), CHAINS[22][2], (CHAINS[22][3], CHAINS[22][4])
        p[0] = (0, 0.95, 0)
        for side, chain in zip((-1, 1), legs):
            for y, j in zip((0.88, 0.5, 0.08, 0.02), chain[1:]):
                p[j] = (0.1 * side, y, 0.12 if y < 0.05 else 0.0)
        for y, j in zip((1.08, 1.22, 1.36, 1.52, 1.66), spine[1:]):
            p[j] = (0, y, 0.02)
        for side, chain in zip((-1, 1), arms):
            for (dx, y), j in zip(((0.08, 1.45), (0.2, 1.42), (0.26, 1.15), (0.28, 0.9)), chain[1:]):
                p[j] = (dx * side, y, 0.0)
    else:
        legs, spine, arms = (CHAINS[21][0], CHAINS[21][1]), CHAINS[21][2], (CHAINS[21][3], CHAINS[21][4])
        p[0] = (0, 0.95, 0)
        for side, chain in zip((-1, 1), legs):
            for y, j in zip((0.9, 0.5, 0.1, 0.04, 0.02), chain[1:]):
                p[j] = (0.1 * side, y, 0.15 if y < 0.03 else (0.08 if y < 0.05 else 0.0))
        for y, j in zip((1.15, 1.35, 1.5, 1.66), spine[1:]):
            p[j] = (0, y, 0.02)
        for side, chain in zip((-1, 1), arms):
            for (dx, y), j in zip(((0.2, 1.42), (0.26, 1.15), (0.28, 0.9)), chain[1:]):
                p[j] = (dx * side, y, 0.0)
    return p


def motion(L, J=22, seed=0, travel=1.0):
    """[L,J,3] float64: the standing pose walking `travel` units along a curved path with a small seeded wobble on every joint."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, L)[:, None]
    x = standing_pose(J)[None] + 0.03 * rng.standard_normal((L, J, 3))
    x[:, :, 0] += 0.3 * travel * np.sin(2.0 * t)
    x[:, :, 2] += travel * t
    x[:, :, 1] += 0.04 * np.abs(np.sin(9.0 * t))
    return x
