"""The CLIP tower's length and route cases (tests/clip_cases.py, run on the GPU by tests/test_gpu_clip_shapes.py) can see the faults they
are meant for.  CPU only: the oracle is the instrument, the library is not loaded.

For every length and route case, on the plain synthetic weights and in fp64, over the DISTINCT prompts of the case (the route cases repeat
prompts; the oracle treats prompts independently, which the second condition checks):

* replacing one token - the first word, a middle word, the last word, of every prompt that has them - moves that prompt's feature by more
  than 10 x the case's f16x3 bound (trained_like.bound with fp16 pairs; the factor of test_encoder_cases.py);
* the feature of every prompt left alone in that run is bit-identical;
* a causal mask that admits key q + 1, one that hides key q - 1 and pooling at EOS - 1 each move every prompt they can apply to by more
  than 10 x the bound, pooling at EOS + 1 every prompt that has a position behind its EOS;
* overwriting the positions behind every prompt's EOS with a smaller id changes nothing (exactly 0).

These are conditions on the INPUTS: a case that misses one gets other lengths or another seed, never another factor.  `pytest -s` prints the
least-moved prompt of every case and fault.  Measured: bounds 9.6e-5 .. 2.3e-4; the least-moved prompt over all cases per fault, as a multiple
of the bound: one token 501 (5 prompts of 77 positions), admit q + 1 679, hide q - 1 928, pool early 8656, pool late 6848.

The argmax, narrow and dedup cases hold prompts without words or with their maximum elsewhere; their pooled positions are asserted here
directly.  On trained-like weights the last word of some prompts moves the output by about 1 x the bound (peaked softmax), which is why the
GPU file runs both weight sets: plain for indexing and masks, trained-like for softmax and LayerNorm."""
import numpy as np
import pytest
import torch

from oracle import ladiff_oracle as orc
from trained_like import bound, oracle_pair

import clip_cases as cc

FACTOR = 10.0
_SD64 = {}


def fp64(ids, **fault):
    if not _SD64:
        _SD64.update({k: v.double() for k, v in cc.weights("plain").items()})
    with torch.no_grad(), cc.faulty(**fault):
        return orc.clip_text_features(_SD64, ids, cc.LAYERS)


@pytest.mark.parametrize("name", cc.names("lengths", "routes"))
def test_case_sees_the_faults_it_exists_for(name):
    c = cc.CASES[name]
    ids = torch.unique(c.ids, dim=0)
    n, S = ids.shape
    eos = ids.argmax(dim=1)
    (want,), (e32,) = oracle_pair(cc.features_fn(ids), cc.weights("plain"))
    b = bound(e32, want, "f16x3", 1)
    assert torch.equal(fp64(ids), want)
    least = {}

    def moved(what, got, applies):
        m = (got - want).abs().amax(dim=1)
        if applies.any():
            least[what] = min(least.get(what, float("inf")), m[applies].min().item())
        assert (m[applies] > FACTOR * b).all(), (name, what, m.tolist(), b)
        return m

    # one token: in run j prompt p is left alone if (p + j) % 4 == 3, else its first / middle / last word changes
    has_words = eos >= 2
    for j in range(4):
        ids2, touched = ids.clone(), torch.zeros(n, dtype=torch.bool)
        for p in range(n):
            which = (p + j) % 4
            if which < 3 and has_words[p]:
                e = int(eos[p])
                at = (1, (1 + e) // 2, e - 1)[which]
                ids2[p, at] = (ids2[p, at] + 101) % (cc.VOCAB - 2)
                touched[p] = True
        got = fp64(ids2)
        moved("token", got, touched)
        assert torch.equal(got[~touched], want[~touched]), (name, j)
    moved("admit q+1", fp64(ids, mask="admit_next"), (eos + 1 < S) | (eos >= 1))          # (a key q + 1 exists for some row up to the EOS)
    moved("hide q-1", fp64(ids, mask="hide_prev"), eos >= 1)
    moved("pool early", fp64(ids, pool=-1), eos >= 1)
    moved("pool late", fp64(ids, pool=1), eos + 1 < S)
    tail = ids.clone()
    for p in range(n):
        tail[p, int(eos[p]) + 1:] = 3
    assert torch.equal(fp64(tail), want), name
    print(f"\n[clip cases] {name}: {n} distinct prompts  e32 {e32:.2e}  f16x3 bound {b:.2e}  least-moved prompt, x the bound: "
          + "  ".join(f"{k} {v / b:.0f}" for k, v in least.items()))


def test_row_counts_sit_on_the_edges():
    """Every row-count edge of csrc/clip.hip's routes is hit exactly, on both sides, ragged and (S = 64, full length) padded."""
    for m in cc.RAGGED_ROWS + cc.SMALL_ROWS + [1]:
        c = cc.CASES[f"ragged{m}"]
        assert cc.rows(c, cc.RAGGED) == m and not c.dedup          # (ragged: the last row of the launch is the last prompt's EOS row)
    assert {256, 257, 1280, 1281, 4095, 4096, 4097, 5376, 5377, 8192, 8193} <= set(cc.RAGGED_ROWS)
    for B in cc.PADDED_B:
        c = cc.CASES[f"padded{B}x64"]
        assert cc.rows(c, cc.FULL) == 64 * B and int(c.ids[-1].argmax()) == 63
    assert {64 * B for B in cc.PADDED_B} >= {256, 1280, 4096, 5376, 8192}
    for B in cc.COUNTS:
        assert cc.CASES[f"prompts{B}"].ids.shape == (B, 12)
    lens = (cc.CASES["mixed"].ids.argmax(dim=1) + 1).tolist()
    assert lens == cc.MIXED_LENS
    for L in cc.UNIFORM:
        assert (cc.CASES[f"uniform{L}"].ids.argmax(dim=1) + 1).tolist() == [L] * 5


def test_argmax_narrow_and_dedup_inputs():
    for row, at in cc.argmax_prompts().values():
        assert int(row.argmax()) == at == int(np.argmax(row.numpy()))
    assert cc.CASES["one_row_alone"].ids.argmax(dim=1).tolist() == [0]
    assert cc.CASES["one_row_in_batch"].ids.argmax(dim=1).tolist() == [4, 0, 39, 1]
    assert cc.CASES["S2"].ids.argmax(dim=1).tolist() == [1, 0, 1, 0, 0]
    ids = cc.CASES["guidance"].ids.numpy()
    uniq, first, inv = np.unique(ids, axis=0, return_index=True, return_inverse=True)
    assert uniq.shape[0] == 4 and first.tolist() != sorted(first.tolist())          # np.unique re-orders the distinct prompts ...
    assert inv.reshape(-1).tolist() == [3, 3, 3, 2, 0, 2, 1, 3, 0]                  # ... and the gather is no identity or sort
    for group in cc.DEDUP_SAME:
        assert all((ids[i] == ids[group[0]]).all() for i in group)
