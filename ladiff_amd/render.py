"""Motions as pictures, on the GPU: joint positions -> stick-figure animation frames and pose strips (csrc/render.hip).

The reference's demo ends in `plot_3d_motion` (data/humanml/utils/plot_script.py: matplotlib, frame by frame, tens of seconds per clip) or
in Blender (`render_batch`).  Here one kernel pair draws the five coloured kinematic chains over the grey ground rectangle - not
matplotlib's pixels: the image model is this library's own, stated in include/ladiff_hip.h and restated in tests/render_ref.py.
`MotionRenderer(...)(joints)` gives one image per frame (root-centred, the ground sliding under the figure), `.strip(joints)` one image
per motion (evenly spaced poses at their true positions, later ones more opaque).  `save_animation` writes what came back."""
import ctypes
import os

import numpy as np
import torch

from . import _lib

MAX_FRAMES, MIN_SIDE, MAX_SIDE = 256, 16, 1024
FRAMES, STRIP = 0, 1                                   # LADIFF_RENDER_FRAMES / LADIFF_RENDER_STRIP
# utils/paramUtil.py: t2m_kinematic_chain (22 joints, HumanML3D) and kit_kinematic_chain (21 joints, KIT-ML)
CHAINS = {22: ((0, 2, 5, 8, 11), (0, 1, 4, 7, 10), (0, 3, 6, 9, 12, 15), (9, 14, 17, 19, 21), (9, 13, 16, 18, 20)),
          21: ((0, 11, 12, 13, 14, 15), (0, 16, 17, 18, 19, 20), (0, 1, 2, 3, 4), (3, 5, 6, 7), (3, 8, 9, 10))}
CHAIN_COLORS = ("#DD5A37", "#D69E00", "#B75A39", "#DD5A37", "#D69E00")      # the first five of plot_3d_motion's list
# line_width None = H / 54: the reference's 4 pt lines on its 3 in x 100 dpi figure
DEFAULTS = dict(elev_deg=15.0, azim_deg=25.0, dist=3.6, focal=2.0, target_height=0.9, near=0.1, line_width=None, ground_margin=0.5,
                alpha_min=0.25, strip_fit=3.0, ground_alpha=0.5, background=(1.0, 1.0, 1.0), ground=(0.5, 0.5, 0.5),
                chain_colors=CHAIN_COLORS)


class RenderParams(ctypes.Structure):
    """`ladiff_render_params` of include/ladiff_hip.h."""
    _fields_ = [("elev_deg", ctypes.c_float), ("azim_deg", ctypes.c_float), ("dist", ctypes.c_float), ("focal", ctypes.c_float),
                ("target_height", ctypes.c_float), ("near_plane", ctypes.c_float), ("line_width", ctypes.c_float),
                ("ground_margin", ctypes.c_float), ("alpha_min", ctypes.c_float), ("strip_fit", ctypes.c_float),
                ("ground_alpha", ctypes.c_float), ("background_rgb", ctypes.c_float * 3), ("ground_rgb", ctypes.c_float * 3),
                ("chain_rgb", (ctypes.c_float * 3) * 5), ("frame_stride", ctypes.c_int32)]


def rgb(colour):
    """'#RRGGBB' or three numbers in [0, 1] -> (r, g, b) floats."""
    if isinstance(colour, str):
        if len(colour) != 7 or colour[0] != "#":
            raise ValueError(f"colour {colour!r}: expected '#RRGGBB'")
        return tuple(int(colour[i:i + 2], 16) / 255.0 for i in (1, 3, 5))
    c = tuple(float(v) for v in colour)
    if len(c) != 3 or any(not 0.0 <= v <= 1.0 for v in c):
        raise ValueError(f"colour {colour!r}: expected three numbers in [0, 1]")
    return c


class MotionRenderer:
    """`MotionRenderer(njoints=22, size=(H, W), **camera_and_style)`: `r(joints[B,L,J,3], lengths) -> [B,L',H,W,3]` (a [L,J,3] input
    gives [L',H,W,3]; L' = ceil(L / frame_stride); images past a motion's length are background) and `r.strip(joints, lengths, n_poses)
    -> [B,H,W,3]`, uint8 or float32 in [0, 1], on the device the joints are on.  1 <= lengths[b] <= L <= 256, 16 <= H, W <= 1024,
    W % 4 == 0.  Camera and style: the keys of `DEFAULTS`.  No CPU implementation: CPU tensors raise."""
    # a frames request is B x L' x H x W x 3 values: 128 motions of 196 frames at 256 x 256 are 4.9 GB as uint8.  Larger requests are
    # refused by name
    max_render_bytes = 8 << 30

    def __init__(self, njoints=22, size=(256, 256), **style):
        if int(njoints) not in CHAINS:
            raise ValueError(f"the renderer knows the 22-joint (HumanML3D) and the 21-joint (KIT) skeleton, got {njoints} joints")
        unknown = sorted(set(style) - set(DEFAULTS))
        if unknown:
            raise TypeError(f"unknown camera / style arguments {unknown}; known: {sorted(DEFAULTS)}")
        self.njoints = int(njoints)
        self.H, self.W = (int(v) for v in size)
        if not (MIN_SIDE <= self.H <= MAX_SIDE and MIN_SIDE <= self.W <= MAX_SIDE) or self.W % 4:
            raise ValueError(f"size (H, W) = {tuple(size)}: sides in [{MIN_SIDE}, {MAX_SIDE}], W a multiple of 4")
        s = {**DEFAULTS, **style}
        if s["line_width"] is None:
            s["line_width"] = self.H / 54.0
        for k in ("elev_deg", "azim_deg", "dist", "focal", "target_height", "near", "line_width", "ground_margin", "alpha_min", "strip_fit",
                  "ground_alpha"):
            s[k] = float(s[k])
        for k in ("dist", "focal", "line_width", "near", "strip_fit"):
            if not s[k] > 0:
                raise ValueError(f"{k} must be positive, got {s[k]}")
        if not abs(s["elev_deg"]) < 90:
            raise ValueError(f"elev_deg must lie inside (-90, 90), got {s['elev_deg']}")
        if not s["target_height"] + s["dist"] * np.sin(np.radians(s["elev_deg"])) > 0:
            raise ValueError("the eye must be above the ground: target_height + dist sin(elev_deg) > 0")
        if not s["ground_margin"] >= 0 or not 0 <= s["alpha_min"] <= 1 or not 0 <= s["ground_alpha"] <= 1:
            raise ValueError("ground_margin >= 0 and alpha_min, ground_alpha in [0, 1]")
        s["background"], s["ground"] = rgb(s["background"]), rgb(s["ground"])
        s["chain_colors"] = tuple(rgb(c) for c in s["chain_colors"])
        if len(s["chain_colors"]) != 5:
            raise ValueError("chain_colors: one colour per kinematic chain, five of them")
        self.style = s

    def params(self, frame_stride=1):
        s = self.style
        p = RenderParams(s["elev_deg"], s["azim_deg"], s["dist"], s["focal"], s["target_height"], s["near"], s["line_width"],
                         s["ground_margin"], s["alpha_min"], s["strip_fit"], s["ground_alpha"])
        p.background_rgb[:], p.ground_rgb[:] = s["background"], s["ground"]
        for i, c in enumerate(s["chain_colors"]):
            p.chain_rgb[i][:] = c
        p.frame_stride = int(frame_stride)
        return p

    def check(self, shape, lengths, dtype=torch.uint8, frame_stride=1, n_poses=None):
        """The argument checks of a call, without a device: shape [L,J,3] or [B,L,J,3]; `n_poses` given = a strip request.  Returns
        (B, L, lengths as ints, the output's shape)."""
        shape = tuple(shape)
        if len(shape) not in (3, 4) or shape[-2:] != (self.njoints, 3):
            raise ValueError(f"joints must be [L, {self.njoints}, 3] or [B, L, {self.njoints}, 3], got {shape}")
        B, L = (1, shape[0]) if len(shape) == 3 else shape[:2]
        if not 1 <= L <= MAX_FRAMES:
            raise ValueError(f"the renderer takes 1 .. {MAX_FRAMES} frames, got {L}")
        if lengths is None:
            lengths = [L] * B
        lengths = [int(l) for l in lengths]
        if len(lengths) != B:
            raise ValueError(f"{len(lengths)} lengths for {B} motions")
        if any(l < 1 or l > L for l in lengths):
            raise ValueError(f"lengths must lie in [1, {L}], got {lengths}")
        if dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"images are torch.uint8 or torch.float32, got {dtype}")
        if int(frame_stride) < 1 or (n_poses is not None and int(n_poses) < 1):
            raise ValueError("frame_stride and n_poses are at least 1")
        out = (B, self.H, self.W, 3) if n_poses is not None else (B, -(-L // int(frame_stride)), self.H, self.W, 3)
        nbytes = int(np.prod(out, dtype=np.int64)) * (1 if dtype == torch.uint8 else 4)
        if nbytes > self.max_render_bytes:
            raise ValueError(f"images {out} as {dtype} are {nbytes} bytes, above max_render_bytes = {self.max_render_bytes}: render fewer "
                             "frames (frame_stride), smaller images (size) or fewer motions per call")
        return B, L, lengths, out

    def _run(self, joints, lengths, dtype, mode, n_poses, frame_stride):
        if not torch.is_tensor(joints):
            raise TypeError("joints must be a tensor")
        if not joints.is_cuda:
            raise _lib.LadiffHipError("libladiff_hip works on GPU tensors only; got a CPU tensor (no CPU fallback exists)")
        B, L, lengths, shape = self.check(joints.shape, lengths, dtype, frame_stride, n_poses if mode == STRIP else None)
        dev = joints.device
        x = joints.detach().to(torch.float32).contiguous()
        out = torch.empty(shape, dtype=dtype, device=dev)
        if B:
            L_ = _lib.lib()
            nbytes = L_.ladiff_render_workspace_bytes(B)
            ws = _lib.workspace(nbytes, dev)
            h_len, p = (ctypes.c_int32 * B)(*lengths), self.params(frame_stride)
            with torch.cuda.device(dev):
                _lib.check(L_.ladiff_render_motion(_lib.ptr(x), h_len, B, L, self.njoints, ctypes.byref(p), mode, int(n_poses), self.H, self.W,
                                                   out.data_ptr(), int(dtype == torch.float32), _lib.ptr(ws), nbytes,
                                                   torch.cuda.current_stream(dev).cuda_stream))
        return out[0] if joints.dim() == 3 else out

    def __call__(self, joints, lengths=None, dtype=torch.uint8, frame_stride=1):
        return self._run(joints, lengths, dtype, FRAMES, 1, frame_stride)

    def strip(self, joints, lengths=None, n_poses=8, dtype=torch.uint8):
        return self._run(joints, lengths, dtype, STRIP, n_poses, 1)


def to_uint8(images):
    """[..., H, W, 3] tensor or array, uint8 or floats in [0, 1] -> a uint8 numpy array on the host (floor(255 c + 0.5), the kernel's rule)."""
    a = images.detach().cpu().numpy() if torch.is_tensor(images) else np.asarray(images)
    if a.dtype != np.uint8:
        a = np.floor(255.0 * np.clip(a.astype(np.float64), 0.0, 1.0) + 0.5).astype(np.uint8)
    if a.ndim not in (3, 4) or a.shape[-1] != 3:
        raise ValueError(f"images must be [H, W, 3] or [L, H, W, 3], got {a.shape}")
    return a


def save_animation(images, path, fps=20):
    """Writes rendered images [L,H,W,3] (or one image [H,W,3]) to `path`: `.npy` (always), `.gif` or `.png` (an APNG when there is more
    than one image) through PIL.  Encoding only - nothing is drawn on the CPU."""
    a = to_uint8(images)
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".npy":
        np.save(str(path), a)
        return str(path)
    if ext not in (".gif", ".png"):
        raise ValueError(f"save_animation writes .gif, .png and .npy, got {path!r}")
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError(f"writing {ext} needs PIL (the Pillow package), which is not installed; '.npy' needs nothing") from e
    frames = [Image.fromarray(f) for f in (a if a.ndim == 4 else a[None])]
    if len(frames) == 1:
        frames[0].save(str(path))
    else:
        frames[0].save(str(path), save_all=True, append_images=frames[1:], duration=max(1, int(round(1000.0 / float(fps)))), loop=0)
    return str(path)
