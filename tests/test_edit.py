"""Motion editing (a loop from a source motion), the parts that need no GPU: `start_step` against diffusers' rule; the three
new C entries in header, exports and binding; their argument errors, returned before any GPU call; the capture key
(tests/edit_key_check.cpp, compiled with AddressSanitizer + UBSan into a stand-alone program that runs as a child process - nothing is
loaded into this interpreter); what LADIFF refuses on the host."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from ladiff_amd import LADIFF, DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, LADiffDenoiser, LADiffVae, _lib
from conftest import ROOT
from test_abi import ABL, DEN_KW, VAE_KW, header_functions
from test_planner import COMPILERS, CSRC

SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -4


def schedulers():
    return [DDIMScheduler(set_alpha_to_one=False, steps_offset=1, clip_sample=False, **SCHED_KW),
            DDPMScheduler(variance_type="fixed_small", clip_sample=False, **SCHED_KW), DPMSolverMultistepScheduler(**SCHED_KW)]


@pytest.mark.parametrize("n", [50, 20, 6])
def test_start_step_is_diffusers_rule(n):
    """diffusers' img2img `get_timesteps`: init_timestep = min(int(n * strength), n), t_start = max(n - init_timestep, 0)."""
    for sch in schedulers():
        for strength in (1.0, 0.999, 0.8, 0.75, 0.6, 0.5, 0.3, 1.0 / 3.0, 0.25, 0.2, 1.0 / n, 1.5 / n):
            want = max(n - min(int(n * strength), n), 0)
            assert 0 <= want < n
            assert sch.start_step(strength, n) == want, (type(sch).__name__, strength, n)
        assert sch.start_step(1.0, n) == 0 and sch.start_step(1.0 / n, n) == n - 1
        for bad in (0.0, -0.5, 1.0001, 2.0, float("nan")):
            with pytest.raises(ValueError, match="strength"):
                sch.start_step(bad, n)
        with pytest.raises(ValueError, match="leaves no step"):
            sch.start_step(0.5 / n, n)                                 # int(n * strength) = 0: nothing would run


@pytest.fixture(scope="module")
def lib():
    from ladiff_amd import build
    build.build()
    return _lib.lib()


NEW = ("ladiff_diffusion_reverse_from", "ladiff_init_latents_from", "ladiff_cfg_scheduler_step_from")


def test_new_entries_are_declared_exported_and_bound(lib):
    for name in NEW:
        assert name in header_functions() and name in _lib.EXPORTS and hasattr(lib, name)
    assert len(lib.ladiff_diffusion_reverse_from.argtypes) == len(lib.ladiff_diffusion_reverse_multistep.argtypes) + 3
    assert len(lib.ladiff_cfg_scheduler_step_from.argtypes) == len(lib.ladiff_cfg_scheduler_step_multistep.argtypes) + 2
    assert lib.ladiff_version() == 6


def test_argument_errors_return_before_any_gpu_call(lib):
    """Host code only: the pointers are never followed (0x1000 is no address of anything)."""
    n = lib.ladiff_denoiser_num_params()
    w = (ctypes.c_void_p * n)(*[0x1000] * n)
    fake, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)

    def reverse(z0=fake, starts=None, first=0, n_steps=6, n_text=1, x0=None):
        return lib.ladiff_diffusion_reverse_from(None, w, None, 0, fake, fake, fake, fake, None, fake, fake, None, 7.5, 1.0, 1, 2, 5, n_text,
                                                 n_steps, fake, fake, 1 << 20, 0, None, None, None, 0, x0, z0, starts, first, None)
    assert reverse(z0=None, starts=fake) == ERR_ARG                    # starts without z0
    assert reverse(first=-1) == ERR_ARG and reverse(first=6) == ERR_ARG and reverse(first=7, starts=fake) == ERR_ARG
    assert reverse(z0=None, first=2) == ERR_ARG                        # a first step without source latents
    assert reverse(z0=odd) == ERR_SHAPE and reverse(starts=ctypes.c_void_p(0x1002)) == ERR_SHAPE
    assert reverse(n_text=2) == ERR_UNSUPPORTED

    init = lambda z0=fake, noise=fake, seeds=None, index=None, first=0, B=2, T=5, starts=None: lib.ladiff_init_latents_from(
        z0, noise, seeds, index, None, fake, starts, first, fake, B, T, None)
    assert init(z0=None) == ERR_ARG and init(noise=None) == ERR_ARG and init(noise=None, index=fake) == ERR_ARG
    assert init(first=-1) == ERR_ARG and init(B=0) == ERR_ARG and init(T=0) == ERR_ARG
    assert init(z0=odd) == ERR_SHAPE and init(starts=ctypes.c_void_p(0x1002)) == ERR_SHAPE

    step = lambda x0=None, first=0, B=2, starts=None: lib.ladiff_cfg_scheduler_step_from(fake, fake, x0, fake, fake, None, 1.0, 0, B, 5,
                                                                                       starts, first, None)
    assert step(first=-1) == ERR_ARG and step(B=0) == ERR_ARG
    assert step(x0=ctypes.c_void_p(0x1008)) == ERR_SHAPE and step(starts=ctypes.c_void_p(0x1002)) == ERR_SHAPE


def test_source_and_starts_in_the_capture_key_under_sanitizers(tmp_path):
    exe = str(tmp_path / "edit_key_check")
    logs = []
    for cxx, extra in COMPILERS:
        cxx = cxx if os.path.isabs(cxx) else shutil.which(cxx)
        if not cxx or not os.path.exists(cxx):
            continue
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *extra, "-I", CSRC,
               os.path.join(ROOT, "tests", "edit_key_check.cpp"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        logs.append(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        if r.returncode == 0:
            break
    else:
        raise AssertionError("no host compiler built the key check with sanitizers:\n" + "\n".join(logs))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


def _pipe(steps=6):
    return LADIFF(denoiser=LADiffDenoiser(ABL, **DEN_KW), vae=LADiffVae(ABL, **VAE_KW),
                  scheduler=DDIMScheduler(set_alpha_to_one=False, steps_offset=1, clip_sample=False, **SCHED_KW), guidance_scale=7.5,
                  num_inference_timesteps=steps, eta=0.0, max_it=5)


def test_python_refuses_on_the_host_what_the_device_could_not_check():
    """The start positions are device data to the loop: LADIFF checks them before anything is uploaded.  The texts here are CPU tensors."""
    pipe, lens = _pipe(), [196, 60, 120]
    text, src = torch.zeros(6, 1, 768), torch.zeros(5, 3, 256)
    run = lambda **kw: pipe._diffusion_reverse(text, lens, **kw)
    with pytest.raises(ValueError, match="for 3 prompts"):
        run(source_latents=src, strength=[0.5, 0.6])                   # strength of the wrong length
    with pytest.raises(ValueError, match="for 3 prompts"):
        run(source_latents=src, start_steps=[1, 2, 3, 4])
    with pytest.raises(ValueError, match="outside a schedule of 6"):
        run(source_latents=src, start_steps=[0, 6, 2])                 # a start >= n
    with pytest.raises(ValueError, match="outside a schedule of 6"):
        run(source_latents=src, start_steps=[0, -1, 2])
    with pytest.raises(ValueError, match="exactly one of"):
        run(source_latents=src, strength=0.5, start_steps=[1, 2, 3])   # both
    with pytest.raises(ValueError, match="exactly one of"):
        run(source_latents=src)                                        # neither
    with pytest.raises(ValueError, match="need source_latents"):
        run(strength=0.5)
    with pytest.raises(ValueError, match="strength"):
        run(source_latents=src, strength=[0.5, 1.5, 0.2])
    with pytest.raises(ValueError, match="source_latents"):
        run(source_latents=torch.zeros(3, 5, 256), strength=0.5)       # [B,T,256] is not the loop's layout
    # what is fine gets as far as the device check
    for kw in (dict(strength=0.5), dict(strength=[1.0, 0.5, 0.2]), dict(start_steps=[0, 5, 3]), dict(start_steps=torch.tensor([0, 5, 3]))):
        with pytest.raises(_lib.LadiffHipError):
            run(source_latents=src, **kw)
    assert pipe._start_steps(3, [1.0, 0.5, 0.2], None) == [0, 3, 5] and pipe._start_steps(2, 0.6, None) == [3, 3]
    with pytest.raises(ValueError, match="exactly one source"):
        model = _pipe()
        model.text_encoder, model.feats2joints = (lambda t: text), (lambda f: f)
        model.edit({"text": ["a"] * 3, "length": lens}, 0.5)
