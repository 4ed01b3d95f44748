"""Per-prompt guidance scale and noise key of one sampling batch, the parts that need no GPU: the C entries exist in header, exports and
binding; their argument errors return before any GPU call; the capture key holds the three arrays by pointer
(tests/prompt_params_key_check.cpp, compiled with AddressSanitizer + UBSan into a stand-alone program that runs as a child process -
nothing is loaded into this interpreter); LADIFF refuses arrays it cannot serve."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from ladiff_amd import LADIFF, DDIMScheduler, LADiffDenoiser, LADiffVae, _lib
from ladiff_amd.distributed import shard_prompt_params, shard_prompts
from conftest import ROOT
from test_abi import ABL, DEN_KW, VAE_KW, header_functions
from test_planner import COMPILERS, CSRC

SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False)
ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from ladiff_amd import build
    build.build()
    return _lib.lib()


def test_new_entries_are_declared_exported_and_bound(lib):
    for name in ("ladiff_diffusion_reverse_prompts", "ladiff_noise_fill_prompts"):
        assert name in header_functions() and name in _lib.EXPORTS and hasattr(lib, name)
    assert len(lib.ladiff_diffusion_reverse_prompts.argtypes) == len(lib.ladiff_diffusion_reverse.argtypes) + 4
    assert lib.ladiff_version() == 6


def test_argument_errors_return_before_any_gpu_call(lib):
    """Host code only: the pointers are never followed (0x1000 is no address of anything)."""
    n = lib.ladiff_denoiser_num_params()
    w = (ctypes.c_void_p * n)(*[0x1000] * n)
    fake = ctypes.c_void_p(0x1000)

    def reverse(init=fake, cfg=1, scales=None, seeds=None, index=None, draw=0):
        return lib.ladiff_diffusion_reverse_prompts(None, w, None, 0, fake, init, fake, fake, None, fake, fake, None, 7.5, 1.0, cfg, 2, 5, 1, 5,
                                                    fake, fake, 1 << 20, 0, scales, seeds, index, draw, None)
    assert reverse(cfg=0, scales=fake) == ERR_ARG                      # per-prompt scales without guidance
    assert reverse(draw=1) == ERR_ARG                                  # the initial noise from seeds that are not there
    assert reverse(init=None, draw=1) == ERR_ARG
    assert reverse(init=None, seeds=fake) == ERR_ARG                   # no tensor and nothing asked to be drawn
    assert reverse(index=fake) == ERR_ARG                              # an index without a key
    assert lib.ladiff_diffusion_reverse(None, w, None, 0, fake, None, fake, fake, None, fake, fake, None, 7.5, 1.0, 1, 2, 5, 1, 5,
                                        fake, fake, 1 << 20, 0, None) == ERR_ARG      # the scalar entry still needs its tensor
    fill = lambda seeds, first_step, T=5: lib.ladiff_noise_fill_prompts(seeds, None, first_step, 1, 2, T, fake, None)
    assert fill(fake, -2) == ERR_ARG and fill(None, 0) == ERR_ARG
    assert fill(fake, -1, T=0) == -2 and fill(fake, -1, T=9) == -2     # LADIFF_ERR_SHAPE, as ladiff_noise_fill


def test_prompt_arrays_in_the_capture_key_under_sanitizers(tmp_path):
    exe = str(tmp_path / "prompt_params_key_check")
    logs = []
    for cxx, extra in COMPILERS:
        cxx = cxx if os.path.isabs(cxx) else shutil.which(cxx)
        if not cxx or not os.path.exists(cxx):
            continue
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *extra, "-I", CSRC,
               os.path.join(ROOT, "tests", "prompt_params_key_check.cpp"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        logs.append(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        if r.returncode == 0:
            break
    else:
        raise AssertionError("no host compiler built the key check with sanitizers:\n" + "\n".join(logs))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "prompt_params_key_check: ok" and r.stderr == "", r.stdout + r.stderr


def _pipe(guidance):
    return LADIFF(denoiser=LADiffDenoiser(ABL, **DEN_KW), vae=LADiffVae(ABL, **VAE_KW),
                  scheduler=DDIMScheduler(set_alpha_to_one=False, steps_offset=1, **SCHED_KW), guidance_scale=guidance,
                  num_inference_timesteps=5, eta=0.0, max_it=5)


def test_arrays_the_model_cannot_serve_are_value_errors():
    """Checked on the host before the device is looked at: the texts here are CPU tensors."""
    lens = [196, 60, 120]
    guided, plain = _pipe(7.5), _pipe(1.0)
    with pytest.raises(ValueError, match="classifier-free"):
        plain._diffusion_reverse(torch.zeros(3, 1, 768), lens, guidance_scale=[2.0, 3.0, 4.0])
    for kw in (dict(guidance_scale=[2.0, 3.0]), dict(seeds=[1, 2, 3, 4]), dict(seeds=[1, 2, 3], prompt_index=[0]),
               dict(guidance_scale=torch.ones(3, 1)), dict(seeds=torch.arange(2))):
        with pytest.raises(ValueError, match="for 3 prompts"):
            guided._diffusion_reverse(torch.zeros(6, 1, 768), lens, **kw)
    with pytest.raises(ValueError, match="needs seeds"):
        guided._diffusion_reverse(torch.zeros(6, 1, 768), lens, prompt_index=[0, 1, 2])
    with pytest.raises(ValueError, match="needs seeds"):
        LADIFF.noise_tensor(None, 1, 3, 5, prompt_index=[0, 1, 2], device="cpu")
    # arrays that are fine get as far as the device check; so does a plain number on an unguided model
    with pytest.raises(_lib.LadiffHipError):
        guided._diffusion_reverse(torch.zeros(6, 1, 768), lens, guidance_scale=[2.0, 3.0, 4.0], seeds=[1, 2 ** 64 - 1, 3], prompt_index=[0, 2 ** 32 - 1, 5])
    with pytest.raises(_lib.LadiffHipError):
        plain._diffusion_reverse(torch.zeros(3, 1, 768), lens, guidance_scale=1.0)


def test_unsigned_values_keep_their_bits():
    s = LADIFF._per_prompt([0, 2 ** 40 + 5, 2 ** 63, 2 ** 64 - 1], 4, "seeds", "u64")
    assert s.dtype == torch.int64 and [int(v) & (2 ** 64 - 1) for v in s] == [0, 2 ** 40 + 5, 2 ** 63, 2 ** 64 - 1]
    i = LADIFF._per_prompt([0, 7, 2 ** 31, 2 ** 32 - 1], 4, "prompt_index", "u32")
    assert i.dtype == torch.int32 and [int(v) & 0xFFFFFFFF for v in i] == [0, 7, 2 ** 31, 2 ** 32 - 1]
    j = LADIFF._per_prompt(torch.tensor([0, 7, 2 ** 31, 2 ** 32 - 1]), 4, "prompt_index", "u32")
    assert torch.equal(i, j)
    g = LADIFF._per_prompt(torch.tensor([1.5, 2.0], dtype=torch.float64), 2, "guidance_scale", "f")
    assert g.dtype == torch.float32 and g.tolist() == [1.5, 2.0]


def test_shard_helper_slices_what_shard_prompts_slices():
    B = 7
    text, lens = torch.arange(2 * B, dtype=torch.float32).reshape(2 * B, 1, 1).expand(2 * B, 1, 768), list(range(10, 10 + B))
    scales, seeds = [1.5 + b for b in range(B)], torch.arange(100, 100 + B)
    seen = []
    for rank in range(3):
        _, sub_lens, _, span = shard_prompts(text, lens, None, rank, 3)
        part = shard_prompt_params(span, guidance_scale=scales, seeds=seeds, prompt_index=None, other=4.0)
        assert len(part["guidance_scale"]) == len(sub_lens) == part["seeds"].numel()
        assert part["prompt_index"] is None and part["other"] == 4.0
        seen += [(l, g, int(s)) for l, g, s in zip(sub_lens, part["guidance_scale"], part["seeds"])]
    assert seen == list(zip(lens, scales, range(100, 100 + B)))
