"""Inputs of the LA-VAE encoder shape cases.  TEST INFRASTRUCTURE ONLY (a plain helper module, like trained_like.py): shared by
tests/test_gpu_encoder_shapes.py (GPU against the fp64 oracle) and tests/test_encoder_cases.py (CPU: the cases can see a wrong key).

The encoder's sequence is [T mu tokens | T logvar tokens | F frames] per sample, S = 2T + F <= 224 rows, M = B S rows per batch; the
key map is 32-bit words over these S positions.  A case = (nfeats, T, frame_per_latent, lengths, F or None = the longest sample, value of
the frames behind every sample's length, seed).  Features are N(0, 1) on EVERY frame of the tensor, those behind a sample's length
included (scaled by `pad_scale`): a masked key that is admitted, or a valid one that is dropped, then moves mu / std."""
from collections import namedtuple

import torch

from ladiff_amd import synthetic as syn
from oracle import ladiff_oracle as orc
from trained_like import trained_like

SEED = 1          # trained_like's seed, as tests/test_gpu_trained_like.py
LENS9 = [196, 60, 120, 1, 77, 196, 48, 150, 33]

Case = namedtuple("Case", "name nfeats T fpl lens F pad_scale seed")


def case(name, lens, nfeats=263, T=5, fpl=48, F=None, pad_scale=1.0, seed=0):
    return Case(name, nfeats, T, fpl, tuple(lens), F or max(lens), pad_scale, seed)


def cycled(B):
    """B lengths: LENS9 cycled, 196 first (S = 206 at T = 5)."""
    return [LENS9[i % len(LENS9)] for i in range(B)]


# T = 5, frame_per_latent = 48.  Word boundaries of the key map: 2T + len = 32, 64, ..., 224 <=> len = 22, 54, 86, 118, 150, 182, 214.
LENGTH_EDGES = [
    ("len1", [1]),                                                            # S = 11
    ("len214", [214]),                                                        # S = 224, the largest sequence
    ("latent_counts", [47, 48, 49, 96, 97, 144, 145, 192, 193]),              # on and beside every latent-count boundary
    ("word_boundaries", [21, 22, 23, 53, 54, 55, 86, 118, 150, 182, 213, 214]),
    ("one_wave_S32", [22]), ("S33", [23]),                                    # the split attention's one-wave variant and its neighbour
    ("one_wave_S32_B3", [22, 22, 5]), ("S33_B3", [23, 22, 5]),
    ("M64", [54]), ("M65", [55]),                                             # split GEMMs: 128-row tiles at M <= 64
]
OVER_PADDED = ("over_padded", [150, 4, 60])                                   # F = 200, the frames behind each length hold values of size 50

# (T, frame_per_latent) other than the shipped (5, 48), and the sequences of fewer than 8 rows each admits
MAX_IT = [(1, 224), (2, 112), (3, 80), (8, 25)]
TINY = [(1, [1]), (1, [3]), (1, [5]), (1, [6]), (2, [1]), (2, [3]), (2, [4]), (3, [1]), (3, [2])]     # S = 3 .. 8
FPL = dict(MAX_IT)


def length_cases(nfeats):
    out = [case(n, l, nfeats) for n, l in LENGTH_EDGES]
    out.append(case(OVER_PADDED[0], OVER_PADDED[1], nfeats, F=200, pad_scale=50.0))
    return out


def features(c):
    """[B, F, nfeats] fp32: N(0, 1), the frames behind each sample's length scaled by pad_scale."""
    g = torch.Generator().manual_seed(7000 + 100 * c.seed + c.nfeats + 31 * len(c.lens) + c.F)
    x = torch.randn(len(c.lens), c.F, c.nfeats, generator=g)
    if c.pad_scale != 1.0:
        for i, l in enumerate(c.lens):
            x[i, l:] *= c.pad_scale
    return x


def eps(c):
    g = torch.Generator().manual_seed(9000 + 100 * c.seed + len(c.lens) + c.T)
    return torch.randn(c.T, len(c.lens), 256, generator=g)


_SD = {}


def weights(kind, nfeats, T):
    """"plain": syn.vae_weights (near-flat softmax: indexing and masks show at full size); "trained": trained_like of them (peaked
    softmax, spread LayerNorm)."""
    key = (kind, nfeats, T)
    if key not in _SD:
        sd = syn.vae_weights(nfeats, max_it=T)
        _SD[key] = sd if kind == "plain" else trained_like(sd, SEED)
    return _SD[key]


def encode_fn(c, x, e, key_lengths=None):
    """fn(dtype, state dict) for trained_like.oracle_pair: (mu, std, latent) of the oracle."""
    return lambda dt, sd: orc.vae_encode(sd, x.to(dt), list(c.lens), e.to(dt), max_it=c.T, frame_per_latent=c.fpl,
                                         key_lengths=key_lengths)
