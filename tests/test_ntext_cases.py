"""The text-sequence cases of the denoiser (tests/ntext_cases.py, run on the GPU by tests/test_gpu_ntext_shapes.py) can see the faults they
are meant for.  CPU only: the oracle is the instrument, the library is not loaded.

For every case of the tokens, latents, rows and masks groups, on both weight sets and in fp64, each modelled fault (ntext_cases.faulty)
moves every sample it applies to by more than 10 x the case's split-mode bound with fp16 pairs (trained_like.bound; 10 is the factor of
test_clip_cases.py / test_encoder_cases.py):

  drop_last    the last text token dropped                                     every sample
  prev_last    the last token of prompt b taken from prompt b - 1              every sample of a batch of more than one
  roll_counts  `counts` rolled by one sample                                   the samples whose count changes
  keep_query   the padded rows' query not zeroed in linear_cross_attention     the samples with a padded row
  near_step    the time tables of a neighbouring step                          every sample

and the oracle under an empty patch gives the unfaulted bits.  On the trained-like weights the two softmaxes that only this route
evaluates are peaked (trained_like.softmax_probe; the smallest over the nine layers of the per-layer mean largest probability):
token-axis softmax (dim 1, over the N tokens per feature) >= 0.35 at every N and >= 0.75 at N <= 3, self-attention over T + N + 1 keys
>= 0.45, largest |logit| of either below 100.

These are conditions on the INPUTS: a case that misses one gets another seed or other counts, never another factor.  `pytest -s` prints
per case e32, the bound, the least-moved sample per fault as a multiple of the bound and the softmax statistics.  Measured: e32 1.2e-6 ..
6.1e-5, bounds 8.1e-5 .. 3.9e-3; the least-moved sample over all cases per fault, as a multiple of the bound, plain / trained-like:
drop_last 191 / 49 (T = 7, N = 77), prev_last 227 / 95, roll_counts 8294 / 855, keep_query 7391 / 865, near_step 4082 / 427; token-axis
softmax 0.38 .. 0.88 (>= 0.79 at N <= 3), self-attention 0.45 (T = 7, N = 77: 0.452) .. 0.92, largest |logit| 85.5."""
import pytest
import torch

from trained_like import bound, oracle_pair, softmax_probe

import ntext_cases as nc

FACTOR = 10.0
_SD64 = {}


def fp64(c, kind, fault=None):
    if kind not in _SD64:
        _SD64[kind] = {k: v.double() for k, v in nc.weights(kind).items()}
    fn = nc.forward_fn(c)
    with torch.no_grad():
        if fault is None:
            return fn(torch.float64, _SD64[kind])
        with nc.faulty(fault):
            return fn(torch.float64, _SD64[kind])


@pytest.mark.parametrize("kind", nc.KINDS)
@pytest.mark.parametrize("name", nc.names("tokens", "latents", "rows", "masks"))
def test_case_sees_the_faults_it_exists_for(name, kind):
    c = nc.CASES[name]
    (want,), (e32,) = oracle_pair(nc.forward_fn(c), nc.weights(kind))
    b = bound(e32, want, "f16x3", 1)
    assert torch.equal(fp64(c, kind), want)
    least = {}
    for fault in nc.FAULTS:
        applies = nc.applies(fault, c)
        moved = (fp64(c, kind, fault) - want).abs().amax(dim=(1, 2))
        if applies.any():
            least[fault] = moved[applies].min().item()
        assert (moved[applies] > FACTOR * b).all(), (name, kind, fault, moved.tolist(), b)
    assert torch.equal(fp64(c, kind), want), name          # the patches are gone
    # every fault applies somewhere unless the case's shape rules it out
    assert "drop_last" in least and "near_step" in least and ("prev_last" in least) == (c.B > 1)
    if c.counts is not None and len(set(c.counts)) > 1:
        assert "roll_counts" in least and "keep_query" in least, (name, c.counts)
    print(f"\n[ntext cases] {name} {kind}: B={c.B} T={c.T} N={c.N} counts={c.counts} t={c.timestep}  e32 {e32:.2e}  f16x3 bound {b:.2e}  "
          "least-moved sample, x the bound: " + "  ".join(f"{k} {v / b:.0f}" for k, v in least.items()))


@pytest.mark.parametrize("name", nc.names("tokens", "latents", "rows", "masks"))
def test_new_softmaxes_are_peaked_on_trained_like_weights(name):
    """Per layer the oracle calls softmax three times: self-attention (dim -1, T + N + 1 keys), the query's features (dim -1, 64) and the
    keys' token axis (dim 1, N)."""
    c = nc.CASES[name]
    _, calls = softmax_probe(lambda: fp64(c, "trained"))
    assert len(calls) == 27
    attn, token = calls[0::3], calls[2::3]
    assert all(p["dim"] == -1 and p["keys"] == c.T + c.N + 1 for p in attn) and all(p["dim"] == 1 and p["keys"] == c.N for p in token)
    tok_top, att_top = min(p["top"] for p in token), min(p["top"] for p in attn)
    logit = max(p["max"] for p in attn + token)
    print(f"\n[ntext cases] {name} trained: token-axis softmax over {c.N}: top {tok_top:.2f} .. {max(p['top'] for p in token):.2f}  "
          f"self-attention over {c.T + c.N + 1} keys: top {att_top:.2f} .. {max(p['top'] for p in attn):.2f}  largest |logit| {logit:.1f}")
    assert tok_top >= (0.75 if c.N <= 3 else 0.35), (name, tok_top)
    assert att_top >= 0.45, (name, att_top)
    assert logit < 100, (name, logit)


def test_counts_differ_between_neighbours():
    """A masked case mixes T, 1 and values between; sample b and sample (b + 1) % B differ wherever the batch allows."""
    for c in nc.CASES.values():
        if c.counts is None or c.name in ("mask_all_T", "mask_all_1"):
            continue
        assert len(c.counts) == c.B and all(1 <= v <= c.T for v in c.counts)
        if c.T == 1 or c.B == 1:
            continue
        assert c.T in c.counts and 1 in c.counts, c
        if c.T > 2 and c.B > 2:
            assert any(1 < v < c.T for v in c.counts), c
        pairs = range(c.B) if not (c.T == 2 and c.B % 2) else range(c.B - 1)
        assert all(c.counts[b] != c.counts[(b + 1) % c.B] for b in pairs), c


def test_groups_sit_on_the_edges():
    by = lambda g: [nc.CASES[n] for n in nc.names(g)]
    assert [c.N for c in by("tokens")] == [2, 3, 4, 16, 63, 64, 65, 76, 77] and all((c.B, c.T) == (4, 5) for c in by("tokens"))
    assert sorted({(c.T, c.N) for c in by("latents")}) == [(T, N) for T in (1, 2, 7, 8) for N in (2, 77)] and all(c.B == 5 for c in by("latents"))
    assert [c.B * c.T for c in by("rows")] == [1, 31, 33, 64, 65, 80, 81] and all(c.N == 2 for c in by("rows"))
    assert [c.timestep for c in by("masks")] == [481, 481, 481, 481, 1, 981]
    assert by("masks")[3].counts is None and by("masks")[4].counts == by("masks")[2].counts == by("garbage")[0].counts
    x0, _ = nc.inputs(by("garbage")[0])
    x1, _ = nc.inputs(by("garbage")[0], garbage=True)
    pad = ~nc.orc.count_mask(by("garbage")[0].counts, 5)
    assert pad.any() and (x0[pad] == 0).all() and (x1[pad] == nc.GARBAGE).all() and torch.equal(x0[~pad], x1[~pad])
