"""Reference of a recorded denoising trajectory for the tests.  The CPU oracle's own schedulers (and the fp64 2M reference
of tests/dpm_solver_ref.py), subclassed: `step` calls the parent, then appends its result - the latents after the step - and the step's
data prediction (x - sqrt(1 - a_t) eps) / sqrt(a_t) from the scheduler's own alphas_cumprod.  They are driven by the oracle's
`diffusion_reverse`; for an edit the same classes go through tests/edit_ref.py's truncation, prompt by prompt.  Nothing of the product is
imported (ladiff_amd.synthetic only makes the weights and inputs, as in tests/edit_ref.py)."""
import torch

from ladiff_amd import synthetic as syn
from oracle import ladiff_oracle as orc
from dpm_solver_ref import DPMSolverPP2M
import edit_ref
import trained_like

BASES = {"ddim": orc.DDIM, "ddpm": orc.DDPM, "dpm": DPMSolverPP2M}
LENS7 = [48, 91, 134, 192, 196, 38, 96]                   # latent counts 1 .. 5: the case of tests/test_gpu_dpm_solver.py
_CACHE = {}


def recording(base):
    class Recording(base):
        def set_timesteps(self, n):
            super().set_timesteps(n)
            self.rec_x, self.rec_x0 = [], []

        def step(self, eps, t, x, *args, **kw):
            out = super().step(eps, t, x, *args, **kw)
            acp = self.alphas_cumprod[int(t)].to(x.dtype)
            self.rec_x.append(out)
            self.rec_x0.append((x - (1 - acp) ** 0.5 * eps) / acp ** 0.5)
            return out
    return Recording


def scheduler(sched):
    return recording(BASES[sched])()


def scheduler_from(sched, start):
    """The recording scheduler that runs positions start .. n - 1 (edit_ref's truncation of the same class)."""
    return edit_ref._from(recording(BASES[sched]), start)


def _rows(rec, lens, T):
    """A scheduler's list of [B,T,256] -> [n,T,B,256] with the rows past each prompt's latent count zeroed: the layout and the mask of z."""
    valid = orc.count_mask(orc.max_iter_elements(lens), T)
    return torch.stack([r.permute(1, 0, 2) * valid.t()[:, :, None].to(r.dtype) for r in rec])


def record(sched, text, lens, noise, steps, dtype=torch.float32, den_sd=None, scale=7.5, eta=0.0, step_noise=None):
    """The loop from noise under the recording scheduler -> (z [T,B,256], latents [n,T,B,256], x0 [n,T,B,256])."""
    sd = orc.cast(syn.denoiser_weights() if den_sd is None else den_sd, dtype)
    sch = scheduler(sched)
    fn = lambda x, t, txt, counts: orc.denoiser_forward(sd, x, t, txt, counts)
    with torch.no_grad():
        z = orc.diffusion_reverse(fn, sch, text.to(dtype), lens, noise.to(dtype), steps, scale, eta,
                                  None if step_noise is None else step_noise.to(dtype))
    T = noise.shape[1]
    return z, _rows(sch.rec_x, lens, T), _rows(sch.rec_x0, lens, T)


def record_edit_prompt(sched, text_rows, length, z0, noise, start, n, scale=7.5):
    """One prompt of an edit alone, as edit_ref.edit_prompt drives it -> (latents [n - start,T,1,256], x0 likewise): positions start .. n - 1."""
    init = edit_ref.noised(sched, n, start, z0, noise)[None]
    sd = syn.denoiser_weights()
    fn = lambda x, t, txt, counts: orc.denoiser_forward(sd, x, t, txt, counts)
    sch = scheduler_from(sched, start)
    with torch.no_grad():
        orc.diffusion_reverse(fn, sch, text_rows, [length], init, n, guidance_scale=scale)
    return _rows(sch.rec_x, [length], z0.shape[0]), _rows(sch.rec_x0, [length], z0.shape[0])


def case7():
    return syn.text_embeddings(7, seed=907), syn.init_noise(LENS7, seed=77)


def oracle_case7(sched, steps=6):
    """The fp64 recording of the seven-prompt case and the oracle's own fp32 error per row: (latents [n,T,7,256] fp64, x0 likewise,
    e32_x [n], e32_x0 [n]) - one run per scheduler and process, shared by the CPU and the GPU tests; nobody writes into it."""
    key = (sched, steps)
    if key not in _CACHE:
        text, noise = case7()

        def fn(dtype, sd):
            _, xs, x0s = record(sched, text, LENS7, noise, steps, dtype, sd)
            return tuple(xs) + tuple(x0s)
        want, e32 = trained_like.oracle_pair(fn, syn.denoiser_weights())
        n = len(want) // 2
        _CACHE[key] = (torch.stack(want[:n]), torch.stack(want[n:]), e32[:n], e32[n:])
    return _CACHE[key]


def prompt_rows(rows, i, lens=LENS7):
    """The valid latent rows of prompt i of one position [T,B,256] -> [count,256]."""
    return rows[:-(-lens[i] // 48), i]


def separation(sched, precision="f16x3", steps=6):
    """What the off-by-one and swap checks of tests/test_gpu_trajectory.py rest on, from the oracle alone.  Per position s: the bound of
    either kind, and the smallest distance (over the prompts' valid rows, max |.| per prompt) of the oracle's row s to its rows s - 1 and
    s + 1 of the same kind and to row s of the other kind -> list of dicts {bx, bx0, near_x, near_x0, swap}."""
    xs, x0s, ex, ex0 = oracle_case7(sched, steps)
    n = xs.shape[0]
    dist = lambda a, b: min((prompt_rows(a, i) - prompt_rows(b, i)).abs().max().item() for i in range(len(LENS7)))
    out = []
    for s in range(n):
        others = [t for t in (s - 1, s + 1) if 0 <= t < n]
        out.append({"bx": trained_like.bound(ex[s], xs[s], precision), "bx0": trained_like.bound(ex0[s], x0s[s], precision),
                    "near_x": min(dist(xs[s], xs[t]) for t in others), "near_x0": min(dist(x0s[s], x0s[t]) for t in others),
                    "swap": dist(xs[s], x0s[s])})
    return out
