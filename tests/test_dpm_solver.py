"""DPMSolverMultistepScheduler on the CPU: its coefficient table against the fp64 reference of tests/dpm_solver_ref.py, the order-1 rows
against the DDIM identity, the sign and the benefit of the second-order term on a problem with a known solution, the guards, and the
argument checks of the two new C entries (host code only: no pointer is followed)."""
import ctypes
import math
import os
import shutil
import subprocess

import pytest
import torch

from ladiff_amd import DDIMScheduler, DPMSolverMultistepScheduler, _lib
from conftest import ROOT
from dpm_solver_ref import DPMSolverPP2M
from test_abi import header_functions
from test_planner import COMPILERS, CSRC

KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
ERR_ARG, ERR_SHAPE = -1, -2


def table_steps(tab, x, es):
    """x' = k_x0 m0 + k_x x + k_m m1 over the rows of `tab`, in fp64 on the table's fp32 values: the latents after every step."""
    tab = tab.to(torch.float64)
    out, m1 = [], None
    for row, e in zip(tab, es):
        sa, sb, kx0, kx, ke, kn, km = [float(v) for v in row[:7]]
        assert ke == 0.0 and kn == 0.0 and float(row[7]) == 0.0
        m0 = (x - sb * e) / sa
        x = kx0 * m0 + kx * x
        if km != 0.0:
            x = x + km * m1
        m1 = m0
        out.append(x)
    return out


@pytest.mark.parametrize("final", ["zero", "sigma_min"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("n", [6, 10, 14, 15, 20, 50])
def test_table_against_the_reference(n, order, final):
    sch = DPMSolverMultistepScheduler(solver_order=order, final_sigmas_type=final, **KW)
    sch.set_timesteps(n)
    ref = DPMSolverPP2M(solver_order=order, final_sigmas_type=final)
    ref.set_timesteps(n)
    assert torch.equal(sch.timesteps, ref.timesteps) and sch.timesteps.dtype == torch.int64
    assert int(sch.timesteps[0]) == 999 and len(sch.timesteps) == n
    tab = sch.coef_table()
    assert tab.shape == (n, _lib.COEF_STRIDE) and tab.dtype == torch.float32 and not sch.needs_noise()
    g = torch.Generator().manual_seed(100 * n + order)
    x = torch.randn(3, 5, 256, generator=g, dtype=torch.float64)
    es = [torch.randn(3, 5, 256, generator=g, dtype=torch.float64) for _ in range(n)]
    got = table_steps(tab, x, es)
    xr = x
    for i, t in enumerate(ref.timesteps):
        xr = ref.step(es[i], t, xr)
        assert torch.allclose(got[i], xr, atol=1e-5, rtol=1e-5), (i, (got[i] - xr).abs().max().item())
    # which rows carry the previous prediction: none at order 1; at order 2 every row but row 0 and, per the rules, the last
    km = tab[:, 6]
    last_first_order = final == "zero" or n < 15
    for i in range(n):
        second = order == 2 and i > 0 and not (i == n - 1 and last_first_order)
        assert (float(km[i]) != 0.0) == second, (i, float(km[i]))
    if final == "zero":
        assert float(tab[-1, 3]) == 0.0 and float(tab[-1, 2]) == 1.0              # written explicitly: x' = m0


@pytest.mark.parametrize("final", ["zero", "sigma_min"])
def test_order_one_is_ddim(final):
    """The known identity: DPM-Solver++ of order 1 is DDIM (eta = 0) between the same two timesteps."""
    n = 20
    sch = DPMSolverMultistepScheduler(solver_order=1, final_sigmas_type=final, **KW)
    sch.set_timesteps(n)
    tab = sch.coef_table().to(torch.float64)
    ddim = DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, **KW)
    acp = ddim.alphas_cumprod.to(torch.float64)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(3, 5, 256, generator=g, dtype=torch.float64)
    e = torch.randn(3, 5, 256, generator=g, dtype=torch.float64)
    ts = [int(t) for t in sch.timesteps]
    for i, s in enumerate(ts):
        a_prev = acp[ts[i + 1]] if i + 1 < n else (torch.tensor(1.0, dtype=torch.float64) if final == "zero" else acp[0])
        x0 = (x - (1 - acp[s]) ** 0.5 * e) / acp[s] ** 0.5
        want = a_prev ** 0.5 * x0 + (1 - a_prev) ** 0.5 * e                        # DDIMScheduler._row at eta = 0: {k_x0, k_eps}
        sa, sb, kx0, kx = [float(v) for v in tab[i, :4]]
        got = kx0 * ((x - sb * e) / sa) + kx * x
        assert float(tab[i, 6]) == 0.0
        assert torch.allclose(got, want, atol=1e-5, rtol=1e-5), (i, (got - want).abs().max().item())


def toy_error(n, order, flip=False):
    """|x_end - exact| per unit |x_T| on data ~ N(0, 0.25 I): eps*(x, acp) = sqrt(1 - acp) x / (0.25 acp + 1 - acp) and the exact
    probability flow x_t = x_T sqrt(var_t / var_T), var = 0.25 acp + 1 - acp.  Everything is linear in x_T: a scalar suffices."""
    sch = DPMSolverMultistepScheduler(solver_order=order, final_sigmas_type="zero", **KW)
    sch.set_timesteps(n)
    tab = sch.coef_table().to(torch.float64)
    acp = sch.alphas_cumprod.to(torch.float64)
    var = lambda a: 0.25 * a + 1.0 - a
    x, m1 = 1.0, None
    for i, t in enumerate(sch.timesteps):
        a = float(acp[int(t)])
        e = math.sqrt(1.0 - a) * x / var(a)
        sa, sb, kx0, kx, _, _, km = [float(v) for v in tab[i, :7]]
        if flip:                                         # the D1 term with the wrong sign: A = k_x0 + k_m stays
            kx0, km = kx0 + 2.0 * km, -km
        m0 = (x - sb * e) / sa
        x = kx0 * m0 + kx * x + (km * m1 if km != 0.0 else 0.0)
        m1 = m0
    exact = math.sqrt(var(1.0) / var(float(acp[int(sch.timesteps[0])])))
    return abs(x - exact)


@pytest.mark.parametrize("n", [20, 40, 80])
def test_second_order_term_helps_and_has_the_right_sign(n):
    e2, e1, ef = toy_error(n, 2), toy_error(n, 1), toy_error(n, 2, flip=True)
    print(f"n = {n}: order 2 {e2:.3e}, order 1 {e1:.3e}, D1 flipped {ef:.3e}, ratio {e2 / e1:.2f}")
    assert e2 <= 0.8 * e1, (e2, e1)
    assert ef > e1, (ef, e1)                             # a sign error in k_m lands on the other side of order 1


def test_guards():
    for bad in (dict(algorithm_type="sde-dpmsolver++"), dict(algorithm_type="dpmsolver"), dict(solver_order=3), dict(use_karras_sigmas=True),
                dict(solver_type="heun"), dict(prediction_type="v_prediction"), dict(thresholding=True), dict(final_sigmas_type="other"),
                dict(timestep_spacing="leading"), dict(euler_at_final=True), dict(beta_schedule="squaredcos_cap_v2"), dict(no_such_option=1)):
        with pytest.raises(NotImplementedError) as info:
            DPMSolverMultistepScheduler(**{**KW, **bad})
        key, value = next(iter(bad.items()))
        assert key in str(info.value) or str(value) in str(info.value), str(info.value)
    sch = DPMSolverMultistepScheduler(**KW)             # diffusers' defaults otherwise: order 2, midpoint, lower_order_final, "zero"
    assert sch.config.solver_order == 2 and sch.config.final_sigmas_type == "zero" and sch.config.lower_order_final
    assert sch.init_noise_sigma == 1.0 and sch.multistep and not sch.needs_noise() and not sch.needs_noise(0.5)
    with pytest.raises(ValueError):
        sch.set_timesteps(1000)                          # linspace(0, 999, 1001).round() repeats a timestep: h = 0
    sch.set_timesteps(999)
    sch.set_timesteps(1)
    assert sch.timesteps.tolist() == [999] and sch.coef_table()[0, 2:4].tolist() == [1.0, 0.0]
    with pytest.raises(ValueError):
        DPMSolverMultistepScheduler(**KW).step(torch.zeros(1, 256), 999, torch.zeros(1, 256))      # before set_timesteps
    assert not getattr(DDIMScheduler(clip_sample=False, **KW), "multistep", False)


def test_config_target_resolves():
    from ladiff_amd import instantiate_from_config
    sch = instantiate_from_config({"target": "diffusers.DPMSolverMultistepScheduler", "params": dict(KW, solver_order=2)})
    assert isinstance(sch, DPMSolverMultistepScheduler)


@pytest.fixture(scope="module")
def lib():
    from ladiff_amd import build
    build.build()
    return _lib.lib()


def test_new_entries_are_declared_and_check_their_arguments_on_the_host(lib):
    """Host code only: the pointers are never followed (0x1000 is no address of anything)."""
    assert len(lib.ladiff_diffusion_reverse_multistep.argtypes) == len(lib.ladiff_diffusion_reverse_prompts.argtypes) + 1
    assert len(lib.ladiff_cfg_scheduler_step_multistep.argtypes) == len(lib.ladiff_cfg_scheduler_step.argtypes) + 1
    assert lib.ladiff_version() == 6
    for name in ("ladiff_diffusion_reverse_multistep", "ladiff_cfg_scheduler_step_multistep"):
        assert name in header_functions() and name in _lib.EXPORTS
    fake = ctypes.c_void_p(0x1000)
    step = lambda B=2, T=5, x0=fake: lib.ladiff_cfg_scheduler_step_multistep(fake, fake, x0, fake, fake, None, 1.0, 0, B, T, None)
    assert step(B=0) == ERR_ARG and step(B=-1) == ERR_ARG and step(T=0) == ERR_ARG and step(x0=None) == ERR_ARG
    assert step(x0=ctypes.c_void_p(0x1004)) == ERR_SHAPE                # 16-byte rows
    n = lib.ladiff_denoiser_num_params()
    w = (ctypes.c_void_p * n)(*[0x1000] * n)

    def reverse(fn, *tail, B=2, T=5):
        return fn(None, w, None, 0, fake, fake, fake, fake, None, fake, fake, None, 7.5, 1.0, 1, B, T, 1, 5, fake, fake, 1 << 20, 0,
                  None, None, None, 0, *tail, None)
    multi, prompts = lib.ladiff_diffusion_reverse_multistep, lib.ladiff_diffusion_reverse_prompts
    assert reverse(multi, fake, B=0) == ERR_ARG and reverse(multi, fake, B=-3) == ERR_ARG
    # a latent count outside 1 .. LADIFF_MAX_LATENTS is refused with the code of the entry it extends
    for T in (0, -1, 99):
        assert reverse(multi, fake, T=T) == reverse(prompts, T=T) == ERR_SHAPE
    assert reverse(multi, ctypes.c_void_p(0x1008)) == ERR_SHAPE


def test_state_buffer_in_the_capture_key_under_sanitizers(tmp_path):
    """tests/dpm_solver_key_check.cpp: csrc/graph_key.h compiled with AddressSanitizer + UBSan into a stand-alone program that runs as a
    child process (nothing is loaded into this interpreter)."""
    exe = str(tmp_path / "dpm_solver_key_check")
    logs = []
    for cxx, extra in COMPILERS:
        cxx = cxx if os.path.isabs(cxx) else shutil.which(cxx)
        if not cxx or not os.path.exists(cxx):
            continue
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *extra, "-I", CSRC,
               os.path.join(ROOT, "tests", "dpm_solver_key_check.cpp"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        logs.append(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        if r.returncode == 0:
            break
    else:
        raise AssertionError("no host compiler built the key check with sanitizers:\n" + "\n".join(logs))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr
