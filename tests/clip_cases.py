"""Token ids of the CLIP text tower's shape cases.  TEST INFRASTRUCTURE ONLY (a plain helper module, like encoder_cases.py): shared by
tests/test_gpu_clip_shapes.py (GPU against the fp64 oracle) and tests/test_clip_cases.py (CPU: the cases can see the faults they exist for).

Vocabulary 512, a 2-layer tower: under the causal mask only the EOS row of the LAST layer reaches the output, so a one-layer tower leaves
the out_proj / fc1 / fc2 / q rows of every other position dead; with two layers every row of layer 0 is a key and a value of layer 1.
Ids have the tokenizer's shape [BOS = vocab - 2, words < vocab - 2, EOS = vocab - 1, EOS padding]; a prompt of n positions has its EOS at
position n - 1 (n = 2: the empty prompt).  `prompt(n, S)` is ONE prompt per (n, S): the route cases repeat prompts (they run with
dedup=False, so every copy is a row range of its own on the device), which keeps the number of DISTINCT prompts - what the CPU conditions
are evaluated on - small.  A case names the layouts it runs in: "ragged" (encode_ids' default), "padded" (ragged=False: every prompt padded
to the batch's longest) and "full" (full_length=True: all S positions)."""
from collections import namedtuple
from contextlib import contextmanager

import torch

from ladiff_amd import synthetic as syn
from oracle import ladiff_oracle as orc
from trained_like import trained_like

VOCAB, LAYERS = 512, 2
BOS, EOS = VOCAB - 2, VOCAB - 1
SEED = 1          # trained_like's seed, as tests/test_gpu_trained_like.py
RAGGED, PADDED, FULL = "ragged", "padded", "full"
ALL = (RAGGED, PADDED, FULL)
LAYOUT_KW = {RAGGED: {}, PADDED: {"ragged": False}, FULL: {"full_length": True}}

Case = namedtuple("Case", "name group ids layouts dedup")


def prompt(n, S=77, variant=0):
    """[S] ids of a prompt of n positions, 2 <= n <= S; deterministic in (n, S, variant)."""
    assert 2 <= n <= S
    g = torch.Generator().manual_seed(7919 * n + 104729 * S + 15485863 * variant)
    row = torch.full((S,), EOS, dtype=torch.int64)
    row[0] = BOS
    row[1:n - 1] = torch.randint(0, VOCAB - 2, (n - 2,), generator=g)
    return row


def ids_of(lens, S=77, distinct=False):
    """[B, S]: prompt b has lens[b] positions.  distinct: prompts of one length differ (variant = the index in the batch)."""
    return torch.stack([prompt(n, S, b + 1 if distinct else 0) for b, n in enumerate(lens)])


def equal_row(value=7, S=77):
    """All positions hold the same id: argmax 0, ONE row, L = 1."""
    return torch.full((1, S), value, dtype=torch.int64)


def fill(total, mix):
    """Prompt lengths that sum to `total` exactly: `mix` cycled while what is left still holds another prompt of >= 2 positions."""
    lens, left, i = [], total, 0
    while left >= mix[i % len(mix)] + 2:
        lens.append(mix[i % len(mix)])
        left -= lens[-1]
        i += 1
    assert 2 <= left <= 78
    lens += [left] if left <= 77 else [39, 39]
    assert sum(lens) == total
    return lens


MIX77 = [77, 77, 33, 77, 77, 64, 77, 9]          # ragged routes: 77-position prompts plus shorter ones
MIX_SMALL = [9, 17, 5, 12]
MIX64 = [64, 20, 45, 33, 9, 2, 57]               # padded routes, S = 64
MIX12 = [2, 3, 5, 12, 7, 9, 4]                   # prompt counts, S = 12

# ---------------------------------------------------------------- 1. lengths, S = 77, all layouts
MIXED_LENS = [2, 3, 17, 31, 32, 33, 34, 63, 64, 65, 66, 76, 77]
UNIFORM = [2, 31, 32, 33, 64, 65, 77]            # 5 prompts of one length: the launch's L itself on each edge


def length_cases():
    out = [Case("mixed", "lengths", ids_of(MIXED_LENS, distinct=True), ALL, False)]
    out += [Case(f"uniform{n}", "lengths", ids_of([n] * 5, distinct=True), ALL, False) for n in UNIFORM]
    return out


# ---------------------------------------------------------------- 2. one-row prompts and narrow ids
def narrow_cases():
    s1 = torch.tensor([[5], [EOS], [BOS], [5], [0]], dtype=torch.int64)
    s2 = torch.tensor([[BOS, EOS], [BOS, 17], [3, 400], [EOS, EOS], [12, 12]], dtype=torch.int64)          # EOS at 1, 0, 1, 0, 0
    return [Case("one_row_alone", "narrow", equal_row(), ALL, True),
            Case("one_row_in_batch", "narrow", torch.cat([ids_of([5]), equal_row(), ids_of([40, 2])]), ALL, True),
            Case("S1", "narrow", s1, ALL, True), Case("S2", "narrow", s2, ALL, True),
            Case("S33", "narrow", ids_of([33, 2, 17, 32], S=33, distinct=True), ALL, True)]


# ---------------------------------------------------------------- 3. argmax semantics
def _words(seed, below):
    return torch.randint(0, below, (77,), generator=torch.Generator().manual_seed(seed))


def argmax_prompts():
    """name -> ([77] ids, pooled position)."""
    low = _words(31, 400)                  # largest id 450 (not vocab - 1) at position 9; ids behind it are words, not padding
    low[0], low[9] = 420, 450
    twice = _words(32, VOCAB - 2)          # vocab - 1 at 5 and at 69 (one lane of clip_eos_kernel sees both): the first counts
    twice[0], twice[5], twice[69] = BOS, EOS, EOS
    late = _words(33, VOCAB - 2)           # the first maximum at 70: the second trip of the lane loop; a smaller peak at 3
    late[0], late[3], late[70] = 400, BOS, EOS
    lanes = _words(34, VOCAB - 2)          # the maximum at 67 and at 70: two lanes tie, the smaller position counts
    lanes[0], lanes[67], lanes[70] = BOS, EOS, EOS
    return {"low": (low, 9), "twice": (twice, 5), "late": (late, 70), "lanes": (lanes, 67)}


def argmax_cases():
    p = argmax_prompts()
    short = ids_of([8])
    out = [Case(f"argmax_{n}", "argmax", torch.cat([row[None], short]), ALL, True) for n, (row, _) in p.items()]
    out.append(Case("argmax_batch", "argmax", torch.cat([row[None] for row, _ in p.values()] + [short]), ALL, True))
    return out


# ---------------------------------------------------------------- 4. row-count routes (dedup=False: the row order is the caller's)
RAGGED_ROWS = [256, 257, 1280, 1281, 4095, 4096, 4097, 5376, 5377, 8192, 8193]
PADDED_B = [4, 5, 20, 21, 64, 65, 84, 85, 128, 129]          # x S = 64: 256, 1280, 4096, 5376, 8192 rows, and one prompt more
SMALL_ROWS = [63, 64, 65, 128, 129]
COUNTS = [1, 3, 4, 5, 63, 64, 65]


def route_cases():
    out = [Case(f"ragged{m}", "routes", ids_of(fill(m, MIX77)), (RAGGED,), False) for m in RAGGED_ROWS]
    for B in PADDED_B:          # the last prompt has 64 positions: its EOS is the last row of the launch
        out.append(Case(f"padded{B}x64", "routes", ids_of([MIX64[i % 7] for i in range(B - 1)] + [64], S=64), (FULL,), False))
    out.append(Case("ragged1", "routes", equal_row(), (RAGGED,), False))
    out += [Case(f"ragged{m}", "routes", ids_of(fill(m, MIX_SMALL)), (RAGGED,), False) for m in SMALL_ROWS]
    for B in COUNTS:
        out.append(Case(f"prompts{B}", "routes", ids_of([MIX12[i % 7] for i in range(B - 1)] + [12], S=12), ALL, False))
    return out


# ---------------------------------------------------------------- 5. dedup
def dedup_case():
    """[""] * 3, a, b, a, c, "", b: np.unique sorts the distinct prompts as b, c, a, "" (first words 100 / 200 / 300, EOS = 511)."""
    empty, a, b, c = prompt(2), prompt(30), prompt(12), prompt(45)
    a[1], b[1], c[1] = 300, 100, 200
    order = [empty, empty, empty, a, b, a, c, empty, b]
    return Case("guidance", "dedup", torch.stack(order), ALL, True)


DEDUP_SAME = [(0, 1, 2, 7), (3, 5), (4, 8)]          # rows of identical prompts


def all_cases():
    out = length_cases() + narrow_cases() + argmax_cases() + route_cases() + [dedup_case()]
    assert len({c.name for c in out}) == len(out)
    return out


CASES = {c.name: c for c in all_cases()}


def names(*groups):
    return [c.name for c in CASES.values() if c.group in groups]


def rows(c, layout):
    """Rows of the device launch of case c in a layout (no duplicate prompts where c.dedup is False)."""
    ids = c.ids if not c.dedup else torch.unique(c.ids, dim=0)
    eos = ids.argmax(dim=1)
    return {RAGGED: int((eos + 1).sum()), PADDED: ids.shape[0] * (int(eos.max()) + 1), FULL: ids.numel()}[layout]


_SD = {}


def weights(kind):
    """"plain": syn.clip_weights (near-flat softmax: indexing and masks show at full size); "trained": trained_like of them."""
    if kind not in _SD:
        sd = syn.clip_weights(VOCAB, LAYERS)
        _SD[kind] = sd if kind == "plain" else trained_like(sd, SEED)
    return _SD[kind]


def features_fn(ids):
    """fn(dtype, state dict) for trained_like.oracle_pair, on the FULL [B, S] ids."""
    return lambda dt, sd: orc.clip_text_features(sd, ids, LAYERS)


@contextmanager
def faulty(mask=None, pool=0):
    """The oracle with a fault, by wrapping the two tensor methods clip_text_features builds its mask and its pooled row with:
    mask "admit_next": query q also sees key q + 1; "hide_prev": query q does not see key q - 1; pool: the pooled position moves by
    `pool` (kept inside 0 .. S - 1: a prompt whose EOS is the last position cannot pool later)."""
    real_triu, real_argmax = torch.Tensor.triu, torch.Tensor.argmax

    def triu(self, diagonal=0):
        if mask == "admit_next":
            return real_triu(self, diagonal + 1)
        m = real_triu(self, diagonal)
        if mask == "hide_prev":
            q = torch.arange(1, self.shape[-1])
            m[q, q - 1] = float("-inf")
        return m

    def argmax(self, *a, **kw):
        return (real_argmax(self, *a, **kw) + pool).clamp(0, self.shape[-1] - 1)

    torch.Tensor.triu, torch.Tensor.argmax = triu, argmax
    try:
        yield
    finally:
        torch.Tensor.triu, torch.Tensor.argmax = real_triu, real_argmax
