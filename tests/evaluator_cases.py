"""Weights, cases and inputs of the T2M evaluator shape tests.  TEST INFRASTRUCTURE ONLY (a plain helper module, like trained_like.py and
encoder_cases.py): shared by tests/test_gpu_evaluator_shapes.py (GPU against the fp64 oracle) and tests/test_evaluator_cases.py (CPU: the
conditions on the inputs below, and that the cases can see the mistakes that matter).

`evaluator_weights(nfeats, regime)` -> (movement, motion, text) state dicts.
* "synthetic" is `syn.t2m_weights(nfeats)` unchanged: Xavier matrices, biases +- 0.02.  Every r / z gate of the GRUs then sits near 0.5 and
  every tanh in its linear part.
* "trained_like" redraws, deterministically in SEED and the CRC of each key (trained_like._gen): every linear, conv and GRU bias
  N(0, BIAS_SIGMA); the head's LayerNorm `output_net.1.*`, whose key has no "norm" in it so that `trained_like.is_layernorm` passes it by,
  as `trained_like.spread_affine` draws gamma / beta; `gru.weight_ih_l0*` and `gru.weight_hh_l0*` times one gain per network;
  `hidden` stays N(0, 1), so the per-direction initial state stays visible.

The gain is the smallest of {2, 3, 4, 6, 8} for which, on the default cases (DEFAULT_MOTION: 5 motions of 196 frames, 49 / 30 / 12 / 49 / 1
movements, nfeats 263; DEFAULT_TEXT: 5 captions of 20 words, lengths 20 / 12 / 5 / 20 / 1), at least a tenth of all r and z gate values
evaluated (sigmoid outputs, valid steps, both directions) lie outside [0.01, 0.99] AND at least a tenth inside [0.1, 0.9]: an all-saturated
GRU hides the n path and z h as well as a flat one does.  Measured with the fp64 oracle restated in tests/test_evaluator_cases.py, which
asserts the two conditions (share outside [0.01, 0.99] | share inside [0.1, 0.9] | e32 of the embedding | max |embedding|):

    motion GRU (H = 1024), synthetic        0.000 | 0.961 | e32 1.7e-6 | max 3.10
    motion GRU, gain 2                      0.057 | 0.638                              (too few saturated)
    motion GRU, gain 3  <- MOTION_GAIN      0.207 | 0.453 | e32 2.2e-6 | max 3.58
    text GRU (H = 512), synthetic           0.000 | 0.998 | e32 1.1e-6 | max 2.63
    text GRU, gain 2                        0.006 | 0.815                              (too few saturated)
    text GRU, gain 3                        0.072 | 0.613                              (too few saturated)
    text GRU, gain 4    <- TEXT_GAIN        0.185 | 0.475 | e32 2.9e-6 | max 3.03

(at gain 8 the shares still hold - motion 0.646 | 0.173, text 0.527 | 0.237 - but e32 reaches 2.5e-4 / 1.8e-4: past the cap of 1e-4 scale that
tests/test_evaluator_cases.py puts on every case, so larger gains are no option either.)

Cases are (name, nfeats, B, F, lens, seed) with F = frames (movement encoder), movements T (motion encoder) or words L (text encoder).
Inputs are N(0, 1) on EVERY row, those behind a sample's length included; the motion encoder's input is the oracle's fp32 movement
encoding of N(0, 1) features of 4 T frames (the same tensor goes to the GPU and to the oracle, so the movement encoder's error does not
compound); POS rows are one-hot.  `pad_fill` overwrites the rows behind each length."""
import zlib
from collections import namedtuple

import torch

from ladiff_amd import synthetic as syn
from oracle import ladiff_oracle as orc
from trained_like import BIAS_SIGMA, _gen, spread_affine

SEED = 1                 # as tests/test_gpu_trained_like.py
MOTION_GAIN = 3.0
TEXT_GAIN = 4.0
GAINS = (2, 3, 4, 6, 8)
REGIMES = ("synthetic", "trained_like")

Case = namedtuple("Case", "name nfeats B F lens seed")


def case(name, lens, F, nfeats=263, seed=0):
    return Case(name, nfeats, len(lens), F, tuple(int(l) for l in lens), seed)


# ---------------------------------------------------------------- weights
def _redraw(sd, seed, gain):
    out = {}
    for key, t in sd.items():
        g = _gen(seed, key)
        leaf = key.split(".")[-1]
        if key.startswith("output_net.1."):
            gamma, beta = spread_affine((int(seed) * 1000003 + zlib.crc32(b"output_net.1")) % (2 ** 63), t.numel())
            out[key] = (gamma if leaf == "weight" else beta).to(t.dtype)
        elif t.dim() == 1 and leaf.startswith("bias"):                      # `bias`, `bias_ih_l0`, `bias_hh_l0_reverse`
            out[key] = (BIAS_SIGMA * torch.randn(t.shape, generator=g)).to(t.dtype)
        elif leaf.startswith(("weight_ih_l0", "weight_hh_l0")):
            out[key] = t * gain
        else:
            out[key] = t.clone()
    assert list(out) == list(sd) and all(out[k].shape == sd[k].shape and out[k].dtype == sd[k].dtype for k in sd)
    return out


_SD = {}


def evaluator_weights(nfeats, regime, seed=SEED, motion_gain=MOTION_GAIN, text_gain=TEXT_GAIN):
    assert regime in REGIMES, regime
    key = (nfeats, regime, seed, motion_gain, text_gain)
    if key not in _SD:
        mv, mo, tx = syn.t2m_weights(nfeats)
        if regime == "trained_like":
            mv, mo, tx = _redraw(mv, seed, 1.0), _redraw(mo, seed, motion_gain), _redraw(tx, seed, text_gain)
        _SD[key] = (mv, mo, tx)
    return _SD[key]


# ---------------------------------------------------------------- length patterns
def patterns(B, T):
    """name -> B lengths in 1 .. T: all 1, all T, decreasing (strictly while T allows: the backward direction then starts at a different
    step for every sample), unsorted with repeats ([9, 18, 4, 18, 1] at B = 5, T = 18), one sample of length T among samples of length 1.
    Patterns that coincide at small B or T are listed once."""
    dec = [max(1, T - (i * (T - 1) + B - 2) // max(1, B - 1)) for i in range(B)] if B > 1 else [T]
    base = [max(1, T // 2), T, max(1, 2 * T // 9), T, 1]
    one = [1] * B
    one[B // 2] = T
    out, seen = [], set()
    for name, lens in (("all1", [1] * B), ("allT", [T] * B), ("decreasing", dec), ("unsorted", [base[i % 5] for i in range(B)]),
                       ("oneT", one)):
        if tuple(lens) not in seen:
            seen.add(tuple(lens))
            out.append((name, lens))
    return out


def cycled(B, lens):
    return [lens[i % len(lens)] for i in range(B)]


# ---------------------------------------------------------------- cases
NFEATS = (263, 251)
MOVE_F = (4, 5, 6, 7, 8, 9, 75, 196)                    # T1 = F / 2 odd or even, T2 = 1, 2, 18, 49
MOVE_B = (1, 3)
MOVE_BIG_B = (41, 42, 83, 84)                           # F = 196: conv0 has 98 B rows (4,018 / 4,116), conv3 and out_net 49 B (4,067 / 4,116)
GRU_T = (1, 2, 18, 49)
GRU_B = (1, 5, 6)                                       # 5, 6: the 4-rows-per-block guard of ln_lrelu, 2 B H over the 256-thread blocks
TEXT_L = (1, 2, 12, 20)
TEXT_B = (1, 5)
BIG_MOTION_LENS = (49, 30, 12, 1)
BIG_TEXT_LENS = (20, 12, 5, 1)

DEFAULT_MOTION = case("default", [49, 30, 12, 49, 1], 49)
DEFAULT_TEXT = case("default", [20, 12, 5, 20, 1], 20)


def movement_cases(nfeats):
    return [case(f"F{F}-B{B}", [F] * B, F, nfeats) for F in MOVE_F for B in MOVE_B]


def movement_big_cases(nfeats):
    return [case(f"F196-B{B}", [196] * B, 196, nfeats) for B in MOVE_BIG_B]


def _gru_cases(Ts, Bs):
    return [case(f"T{T}-B{B}-{name}", lens, T) for T in Ts for B in Bs for name, lens in patterns(B, T)]


def motion_cases():
    return _gru_cases(GRU_T, GRU_B)


def text_cases():
    return _gru_cases(TEXT_L, TEXT_B)


def motion_big_case(nfeats=263):
    return case("T49-B84-cycled", cycled(84, BIG_MOTION_LENS), 49, nfeats)


def text_big_case():
    return case("L20-B205-cycled", cycled(205, BIG_TEXT_LENS), 20)


def by_name(cases, name):
    return next(c for c in cases if c.name == name)


# ---------------------------------------------------------------- inputs
def _g(c, salt):
    return torch.Generator().manual_seed(salt + 100003 * c.seed + 1009 * c.nfeats + 31 * c.B + c.F + zlib.crc32(repr(c.lens).encode()) % 9973)


def features(c, frames=None):
    """[B, frames or F, nfeats] fp32, N(0, 1) on every frame."""
    return torch.randn(c.B, frames or c.F, c.nfeats, generator=_g(c, 7000))


_MOV = {}


def movements(c, regime):
    """[B, T, 512] fp32: the oracle's movement encoding (fp32) of N(0, 1) features of 4 T frames under `regime`'s movement weights."""
    key = (c, regime)
    if key not in _MOV:
        with torch.no_grad():
            _MOV[key] = orc.t2m_movement_encoder(evaluator_weights(c.nfeats, regime)[0], features(c, 4 * c.F)).contiguous()
    return _MOV[key]


def words(c):
    """([B, L, 300] N(0, 1), [B, L, 15] one-hot), padding rows included."""
    g = _g(c, 8000)
    w = torch.randn(c.B, c.F, 300, generator=g)
    pos = torch.nn.functional.one_hot(torch.randint(0, 15, (c.B, c.F), generator=g), 15).float()
    return w, pos


def pad_fill(x, lens, value):
    """A copy of x [B, T, ...] whose rows behind each sample's length hold `value`."""
    y = x.clone()
    for i, l in enumerate(lens):
        y[i, l:] = value
    return y


# ---------------------------------------------------------------- oracle functions for trained_like.oracle_pair
def movement_fn(x):
    return lambda dt, mv: orc.t2m_movement_encoder(mv, x.to(dt))


def motion_fn(mov, lens):
    return lambda dt, mo: orc.t2m_motion_encoder(mo, mov.to(dt), list(lens))


def text_fn(w, pos, lens):
    return lambda dt, tx: orc.t2m_text_encoder(tx, w.to(dt), pos.to(dt), list(lens))


def chain_fn(x, lens):
    def fn(dt, mv, mo):
        mov = orc.t2m_movement_encoder(mv, x.to(dt))
        return mov, orc.t2m_motion_encoder(mo, mov, list(lens))
    return fn
