"""Reference of an edit (a loop from a source motion) for the tests, prompt by prompt: the CPU oracle's own reverse loop
with B = 1 under a scheduler whose `set_timesteps` keeps `num_inference_steps = n` but truncates `timesteps` to `[s:]`, fed
`init_noise = alpha(s) z0 + sigma(s) noise` computed here in torch and the step noise of the same positions, then the oracle's decoder.
The multistep form is tests/dpm_solver_ref.DPMSolverPP2M truncated the same way: its step counter starts at 0 on the truncated list, so
the first step taken is first order - the solver restarted at s.  Nothing of the product is imported."""
import torch

from ladiff_amd import synthetic as syn
from oracle import ladiff_oracle as orc
from dpm_solver_ref import DPMSolverPP2M


def _from(base, start):
    class From(base):
        def set_timesteps(self, n):
            super().set_timesteps(n)
            self.full_timesteps = self.timesteps
            self.timesteps = self.timesteps[start:]
    return From()


def scheduler_from(sched, start):
    """`sched` in "ddim" | "ddpm" | "dpm": the oracle's scheduler (or the fp64 2M reference) that runs positions start .. n - 1."""
    return _from({"ddim": orc.DDIM, "ddpm": orc.DDPM, "dpm": DPMSolverPP2M}[sched], start)


def noised(sched, n, start, z0, noise):
    """scheduler.add_noise(z0, noise, timesteps[start]) of an n-step schedule, fp32 on the scheduler's own alphas_cumprod.  z0, noise: [T,256]."""
    s = scheduler_from(sched, 0)
    s.set_timesteps(n)
    acp = s.alphas_cumprod[int(s.timesteps[start])].to(torch.float32)
    return acp ** 0.5 * z0.to(torch.float32) + (1 - acp) ** 0.5 * noise.to(torch.float32)


def generator_noise(seed, index, n, T):
    """What the per-prompt device generator draws for (seed, index): (initial noise [T,256] at position -1, step noise [n,1,T,256])."""
    init = torch.from_numpy(orc.device_noise(seed, index, 2 ** 32 - 1, 1, 1, T))[0, 0]
    return init, torch.from_numpy(orc.device_noise(seed, index, 0, n, 1, T))


def edit_prompt(text_rows, length, z0, noise, start, n, sched, scale, step_noise=None):
    """One prompt alone.  text_rows [2,1,768] (unconditional first) or [1,1,768] with scale <= 1; z0, noise [T,256]; step_noise
    [n,1,T,256] of the FULL schedule or None.  -> (z [T,1,256], frames [1,length,263])."""
    init = noised(sched, n, start, z0, noise)[None]
    sd = syn.denoiser_weights()
    fn = lambda x, t, txt, counts: orc.denoiser_forward(sd, x, t, txt, counts)
    z = orc.diffusion_reverse(fn, scheduler_from(sched, start), text_rows, [length], init, n, guidance_scale=scale,
                              step_noise=None if step_noise is None else step_noise[start:])
    return z, orc.vae_decode(syn.vae_weights(263), z, [length])
