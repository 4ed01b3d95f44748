"""Shape cases of the denoiser with a text SEQUENCE per prompt (`clip_hidden` / `bert` conditioning, mld_clip.py:80-86: N > 1 tokens).
TEST INFRASTRUCTURE ONLY (a plain helper module, like clip_cases.py): shared by tests/test_gpu_ntext_shapes.py (GPU against the fp64
oracle) and tests/test_ntext_cases.py (CPU: the cases can see the faults they exist for).

N > 1 runs code no other route runs: csrc/linear_ca.hip (lca_kv_kernel: softmax over the N tokens per feature; lca_apply_kernel: softmax
over the 64 features per head, padded rows' query zeroed; den_self_attn_general_kernel: T + N + 1 keys), denoiser_text_cache_general and
the `ntxt > 1` branches of denoiser_forward.  A case is (name, group, B, T, N, counts | None, timestep); B is the batch the network sees
(the loop's duplicated batch).  Its inputs come from a generator seeded by the CRC of its name.  The groups:

  tokens   B = 4, T = 5, N = 2, 3, 4, 16, 63, 64, 65, 76, 77: the smallest N, the 64-lane / 256-thread strides of lca_kv_kernel's load loop
           (N x 64 values over 256 threads), the limit LADIFF_CLIP_MAX_POSITIONS
  latents  B = 5, T = 1, 2, 7, 8 at N = 2 and 77: the kernels are instantiated for TMAX = 8 with `t < T` guards
  rows     N = 2, (B, T) = (1,1) (31,1) (33,1) (16,4) (13,5) (16,5) (27,3): M = B T = 1, 31 / 33, 64 / 65, 80 / 81 - both sides of the row
           tiles launch_gemm_kr picks (<32,32>, <64,64>, <80,64>), which gemm_rowln passes too in split mode
  masks    B = 6, T = 5, N = 3: counts all T, all 1, mixed, None; the mixed one also at timesteps 1 and 981 (every other case: 481)
  garbage  the mixed-mask case whose latent rows t >= counts[b] hold 1e30 (`inputs(c, garbage=True)`; `inputs(c)` has zeros there)

`counts` of a masked case cycles through T, 1, 2 .. T - 1: neighbours differ, and sample b differs from sample (b + 1) % B wherever B and T
allow it (T = 1 allows one value; T = 2 with an odd B leaves the last and the first sample equal), so a count read from another sample
changes something.

`faulty(kind)` patches the oracle (oracle/ladiff_oracle.py) with one modelled fault, for the CPU file:
  "drop_last"    the last text token is dropped
  "prev_last"    the last token of prompt b is taken from prompt b - 1 (prompt 0: from the last prompt)
  "roll_counts"  `counts` rolled by one sample
  "keep_query"   the padded rows' query is not zeroed in linear_cross_attention
  "near_step"    the time tables of a neighbouring step (timestep - 20; + 20 below 20)
`applies(kind, c)` is the [B] mask of the samples a fault can move."""
import zlib
from collections import namedtuple
from contextlib import contextmanager

import torch

from ladiff_amd import synthetic as syn
from oracle import ladiff_oracle as orc
from trained_like import trained_like

SEED = 1          # trained_like's seed, as tests/test_gpu_trained_like.py
TIMESTEP = 481
GARBAGE = 1e30
KINDS = ("plain", "trained")
FAULTS = ("drop_last", "prev_last", "roll_counts", "keep_query", "near_step")

Case = namedtuple("Case", "name group B T N counts timestep")

TOKENS_N = [2, 3, 4, 16, 63, 64, 65, 76, 77]
LATENTS_T = [1, 2, 7, 8]
ROWS_BT = [(1, 1), (31, 1), (33, 1), (16, 4), (13, 5), (16, 5), (27, 3)]


def mixed_counts(B, T):
    """[B] counts cycling through T, 1, 2 .. T - 1; the last sample moved off the first one's value where another value is left."""
    vals = list(dict.fromkeys([T, 1] + list(range(2, T))))
    c = [vals[b % len(vals)] for b in range(B)]
    if B > 2 and c[-1] == c[0]:
        for v in vals:
            if v != c[0] and v != c[-2]:
                c[-1] = v
                break
    return c


def all_cases():
    out = [Case(f"tokens{N}", "tokens", 4, 5, N, mixed_counts(4, 5), TIMESTEP) for N in TOKENS_N]
    out += [Case(f"latents{T}_N{N}", "latents", 5, T, N, mixed_counts(5, T), TIMESTEP) for T in LATENTS_T for N in (2, 77)]
    out += [Case(f"rows{B}x{T}", "rows", B, T, 2, mixed_counts(B, T), TIMESTEP) for B, T in ROWS_BT]
    mixed = mixed_counts(6, 5)
    out += [Case("mask_all_T", "masks", 6, 5, 3, [5] * 6, TIMESTEP), Case("mask_all_1", "masks", 6, 5, 3, [1] * 6, TIMESTEP),
            Case("mask_mixed", "masks", 6, 5, 3, mixed, TIMESTEP), Case("mask_none", "masks", 6, 5, 3, None, TIMESTEP),
            Case("mask_mixed_t1", "masks", 6, 5, 3, mixed, 1), Case("mask_mixed_t981", "masks", 6, 5, 3, mixed, 981)]
    out.append(Case("garbage", "garbage", 6, 5, 3, mixed, TIMESTEP))
    assert len({c.name for c in out}) == len(out)
    return out


CASES = {c.name: c for c in all_cases()}


def names(*groups):
    return [c.name for c in CASES.values() if c.group in groups]


def generator(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def counts_of(c):
    return None if c.counts is None else torch.tensor(c.counts)


def inputs(c, garbage=False):
    """(sample [B,T,256], text [B,N,768]) of case c, fp32.  The garbage case has zeros in its padded latent rows, or 1e30 on request."""
    g = generator(c.name)
    x, txt = torch.randn(c.B, c.T, 256, generator=g), torch.randn(c.B, c.N, 768, generator=g)
    if c.group == "garbage":
        pad = ~orc.count_mask(c.counts, c.T)
        x[pad] = GARBAGE if garbage else 0.0
    return x, txt


_SD = {}


def weights(kind):
    """"plain": syn.denoiser_weights (near-flat softmax: indexing and masks show at full size); "trained": trained_like of them."""
    if kind not in _SD:
        sd = syn.denoiser_weights()
        _SD[kind] = sd if kind == "plain" else trained_like(sd, SEED)
    return _SD[kind]


def forward_fn(c):
    """fn(dtype, state dict) for trained_like.oracle_pair: the denoiser forward of case c."""
    x, txt = inputs(c)
    counts = counts_of(c)
    return lambda dt, sd: orc.denoiser_forward(sd, x.to(dt), c.timestep, txt.to(dt), counts)


def block_params(sd, layer):
    """The ca_block parameters of layer 0 .. 8 (the order of the library's weight table: input blocks, middle block, output blocks)."""
    return orc.sub(sd, f"encoder.{orc.block_names()[layer]}.ca_block")


def near_step(t):
    t = torch.as_tensor(t)
    return torch.where(t >= 20, t - 20, t + 20)


def applies(kind, c):
    """[B] bool: the samples of case c that fault `kind` can move."""
    every = torch.ones(c.B, dtype=torch.bool)
    if kind == "prev_last":
        return every if c.B > 1 else ~every
    if kind == "roll_counts":
        return ~every if c.counts is None else torch.tensor(c.counts).roll(1) != torch.tensor(c.counts)
    if kind == "keep_query":
        return ~every if c.counts is None else torch.tensor(c.counts) < c.T
    assert kind in ("drop_last", "near_step"), kind
    return every


@contextmanager
def faulty(kind):
    """The oracle with one modelled fault (see the module's docstring): the functions denoiser_forward reaches by their module names
    are replaced while the block runs."""
    assert kind in FAULTS, kind
    real = {n: getattr(orc, n) for n in ("skip_encoder", "count_mask", "linear_cross_attention", "time_embedding")}

    def skip_encoder(x, xf, emb, p, pad_mask, num_layers=9):
        if kind == "drop_last":
            xf = xf[:, :-1]
        else:
            last = xf.roll(1, 0)[:, -1].clone()
            xf = xf.clone()
            xf[:, -1] = last
        return real["skip_encoder"](x, xf, emb, p, pad_mask, num_layers)

    def count_mask(counts, n):
        return real["count_mask"](torch.as_tensor(counts).roll(1), n)

    def linear_cross_attention(x, xf, emb, p, pad_mask, num_heads=orc.NUM_HEADS):
        return real["linear_cross_attention"](x, xf, emb, p, None, num_heads)

    def time_embedding(sd, t, dtype=torch.float32):
        return real["time_embedding"](sd, near_step(t), dtype)

    patch = {"drop_last": ("skip_encoder", skip_encoder), "prev_last": ("skip_encoder", skip_encoder), "roll_counts": ("count_mask", count_mask),
             "keep_query": ("linear_cross_attention", linear_cross_attention), "near_step": ("time_embedding", time_embedding)}[kind]
    setattr(orc, *patch)
    try:
        yield
    finally:
        setattr(orc, patch[0], real[patch[0]])
