"""The denoising trajectory, the parts that need no GPU: the two new C entries in header, exports and binding and their
argument errors; the capture key and the launch policy of a recording call (tests/trajectory_key_check.cpp under sanitizers, as a
stand-alone child process); what LADIFF refuses on the host; the reference recorder of tests/trajectory_ref.py against the oracle's own
loop; and the separation the off-by-one checks of tests/test_gpu_trajectory.py rest on, from the oracle alone."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from ladiff_amd import LADIFF, DDIMScheduler, LADiffDenoiser, LADiffVae, _lib, synthetic as syn
from oracle import ladiff_oracle as orc
from conftest import ROOT
from dpm_solver_ref import DPMSolverPP2M
from test_abi import ABL, DEN_KW, VAE_KW, header_functions
from test_planner import COMPILERS, CSRC
import trajectory_ref as ref

SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -4


@pytest.fixture(scope="module")
def lib():
    from ladiff_amd import build
    build.build()
    return _lib.lib()


def test_new_entries_are_declared_exported_and_bound(lib):
    for name in ("ladiff_diffusion_reverse_record", "ladiff_cfg_scheduler_step_record"):
        assert name in header_functions() and name in _lib.EXPORTS and hasattr(lib, name)
    assert len(lib.ladiff_diffusion_reverse_record.argtypes) == len(lib.ladiff_diffusion_reverse_from.argtypes) + 2
    assert len(lib.ladiff_cfg_scheduler_step_record.argtypes) == len(lib.ladiff_cfg_scheduler_step_from.argtypes) + 2
    assert lib.ladiff_version() == 6


def test_argument_errors_return_before_any_gpu_call(lib):
    """Host code only: the pointers are never followed (0x1000 is no address of anything)."""
    n = lib.ladiff_denoiser_num_params()
    w = (ctypes.c_void_p * n)(*[0x1000] * n)
    fake, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008)

    def reverse(tx=fake, tx0=fake, z0=None, starts=None, first=0, n_text=1):
        return lib.ladiff_diffusion_reverse_record(None, w, None, 0, fake, fake, fake, fake, None, fake, fake, None, 7.5, 1.0, 1, 2, 5, n_text,
                                                   6, fake, fake, 1 << 20, 0, None, None, None, 0, None, z0, starts, first, tx, tx0, None)
    assert reverse(tx=odd) == ERR_SHAPE and reverse(tx0=odd) == ERR_SHAPE and reverse(tx=None, tx0=odd) == ERR_SHAPE
    assert reverse(n_text=2) == ERR_UNSUPPORTED and reverse(tx=None, n_text=2) == ERR_UNSUPPORTED
    assert reverse(starts=fake) == ERR_ARG and reverse(first=2) == ERR_ARG       # the edit's own rules still hold

    step = lambda tx=fake, tx0=fake, first=0, B=2: lib.ladiff_cfg_scheduler_step_record(fake, fake, None, fake, fake, None, 1.0, 0, B, 5, None,
                                                                                      first, tx, tx0, None)
    assert step(first=-1) == ERR_ARG and step(B=0) == ERR_ARG
    assert step(tx=odd) == ERR_SHAPE and step(tx0=odd) == ERR_SHAPE


def test_buffers_in_the_capture_key_under_sanitizers(tmp_path):
    exe = str(tmp_path / "trajectory_key_check")
    logs = []
    for cxx, extra in COMPILERS:
        cxx = cxx if os.path.isabs(cxx) else shutil.which(cxx)
        if not cxx or not os.path.exists(cxx):
            continue
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *extra, "-I", CSRC,
               os.path.join(ROOT, "tests", "trajectory_key_check.cpp"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        logs.append(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        if r.returncode == 0:
            break
    else:
        raise AssertionError("no host compiler built the key check with sanitizers:\n" + "\n".join(logs))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


def _pipe(steps=6, **kw):
    return LADIFF(denoiser=LADiffDenoiser(ABL, **DEN_KW), vae=LADiffVae(ABL, **VAE_KW),
                  scheduler=DDIMScheduler(set_alpha_to_one=False, steps_offset=1, clip_sample=False, **SCHED_KW), guidance_scale=7.5,
                  num_inference_timesteps=steps, eta=0.0, max_it=5, **kw)


def test_python_refuses_on_the_host():
    """Every argument error of a recording call is raised before any GPU work: the texts here are CPU tensors."""
    pipe, lens = _pipe(), [196, 60, 120]
    text = torch.zeros(6, 1, 768)
    for bad in ("x", "latent", "all", True, 1):
        with pytest.raises(ValueError, match="trajectory"):
            pipe._diffusion_reverse(text, lens, trajectory=bad)
        with pytest.raises(ValueError, match="trajectory"):
            pipe.sample(text, lens, trajectory=bad)
    with pytest.raises(NotImplementedError, match="test_efficiency"):
        _pipe(test_efficiency=True)._diffusion_reverse(text, [60, 60, 60], trajectory="x0")
    with pytest.raises(NotImplementedError, match="n_text"):
        pipe._diffusion_reverse(torch.zeros(6, 2, 768), lens, trajectory="latents")
    # the size: n x B x T KiB per kind, named in the message
    small = _pipe()
    small.max_trajectory_bytes = 6 * 3 * 5 * 1024                     # exactly one kind of this call
    with pytest.raises(ValueError, match=str(2 * 6 * 3 * 5 * 1024)):
        small._diffusion_reverse(text, lens, trajectory="both")
    with pytest.raises(_lib.LadiffHipError):                          # what fits gets as far as the device check
        small._diffusion_reverse(text, lens, trajectory="x0")
    assert LADIFF.max_trajectory_bytes == 1 << 30
    big = _pipe(steps=1000)
    with pytest.raises(ValueError, match=str(2 * 1000 * 128 * 5 * 1024)):
        big._diffusion_reverse(torch.zeros(256, 1, 768), [196] * 128, trajectory="both")     # 655 MB per kind: one fits, two do not
    with pytest.raises(_lib.LadiffHipError):
        big._diffusion_reverse(torch.zeros(256, 1, 768), [196] * 128, trajectory="latents")
    with pytest.raises(ValueError, match="kind"):
        pipe.preview({"text": ["a"] * 3, "length": lens}, kind="both")
    with pytest.raises(ValueError, match="expected"):
        pipe.decode_trajectory(torch.zeros(6, 5, 2, 256), lens)
    with pytest.raises(ValueError, match="outside a trajectory of 6"):
        pipe.decode_trajectory(torch.zeros(6, 5, 3, 256), lens, steps=[0, 6])


@pytest.mark.parametrize("sched", ["ddim", "ddpm", "dpm"])
def test_recorder_ends_at_the_oracles_own_result(sched):
    """The helper's last row times the valid mask is the z of the oracle's own loop under the plain scheduler; every row has z's layout."""
    lens, steps = [48, 130, 196], 4
    text, noise = syn.text_embeddings(3, seed=5), syn.init_noise(lens, seed=6)
    plain = {"ddim": orc.DDIM, "ddpm": orc.DDPM, "dpm": DPMSolverPP2M}[sched]()
    plain.set_timesteps(steps)
    n = len(plain.timesteps)
    step_noise = torch.randn(n, 3, 5, 256, generator=torch.Generator().manual_seed(7)) if sched == "ddpm" else None
    sd = syn.denoiser_weights()
    fn = lambda x, t, txt, counts: orc.denoiser_forward(sd, x, t, txt, counts)
    with torch.no_grad():
        want = orc.diffusion_reverse(fn, plain, text, lens, noise, steps, step_noise=step_noise)
    z, xs, x0s = ref.record(sched, text, lens, noise, steps, step_noise=step_noise)
    assert xs.shape == x0s.shape == (n, 5, 3, 256)
    assert torch.equal(z, want) and torch.equal(xs[-1], want)
    for i, l in enumerate(lens):
        c = -(-l // 48)
        assert c == 5 or (xs[:, c:, i].abs().max().item() == 0 and x0s[:, c:, i].abs().max().item() == 0)
        assert xs[:, :c, i].abs().min(dim=-1).values.max().item() > 0


@pytest.mark.parametrize("sched", ["ddim", "dpm"])
def test_oracle_rows_are_far_apart_where_the_gpu_test_tells_them_apart(sched):
    """Seven prompts, 6 steps: a row of the oracle's record is at least 10 bounds (f16x3, the wider one) away from its neighbours of the
    same kind and from the row of the other kind - except the last DPM row, whose latents ARE its data prediction (sigma = 0)."""
    sep = ref.separation(sched, "f16x3")
    assert len(sep) == 6
    for s, d in enumerate(sep):
        print(f"{sched} position {s}: bound x {d['bx']:.2e} x0 {d['bx0']:.2e}; nearest neighbour row x {d['near_x']:.3g} x0 {d['near_x0']:.3g}; "
              f"|x - x0| {d['swap']:.3g}")
        assert d["near_x"] >= 10 * d["bx"] and d["near_x0"] >= 10 * d["bx0"]
        if sched == "dpm" and s == 5:
            assert d["swap"] == 0.0
        else:
            assert d["swap"] >= 10 * max(d["bx"], d["bx0"])
