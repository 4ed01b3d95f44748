"""MldTextEncoder.encode_ids against the fp64 oracle over the layouts, lengths and row counts that decide which code runs
(csrc/clip.hip, the attention forms of csrc/attention.hip, the GEMM routes of csrc/gemm.hip / gemm_big.hip / gemm_kr.hip).

* three row layouts: ragged (prompt b owns rows row_off[b] .. row_off[b + 1] - 1, the EOS found on the host), padded to the batch's
  longest prompt and full length (the EOS found by clip_eos_kernel on the device);
* causal attention through the decoder's kernels: the split mode's one-wave form at L <= 32 of the LAUNCH, 32-key map words;
* GEMM routes by row count M: split mode K-resident 64x64 tiles + partial planes at M <= 256, gemm_big_split above (64-row tiles up to
  M = 1280 for fc1 and 5376 for the N = 768 products), fc2 in K parts up to M = 8192; fp32 mode staged tiles below M = 4096, gemm_big
  from there; the final projection is an fp32 GEMM of B rows; the row kernels take four rows per workgroup;
* host work: np.unique dedup and the gather back, argmax = first occurrence of the largest id, Lx = max EOS + 1, the packed meta vector.

Cases: tests/clip_cases.py (vocabulary 512, 2 layers - a one-layer tower leaves most rows dead).  Every case runs on both weight sets and
in both precisions in each layout it names, against the fp64 oracle on the FULL [B, S] ids, within trained_like.bound (fp32: 8 e32 +
1e-6 scale; split mode 8 x (fp16 pairs) / 256 x (bf16 pairs) the e32 term; e32 = the oracle's own fp32-vs-fp64 difference of the case);
a second call gives the same bits.  On the plain weights one changed token, one wrongly admitted or hidden key and a pooled row off by one
each move a prompt by > 10 x the f16x3 bound (tests/test_clip_cases.py); on the trained-like ones softmax is peaked and the LayerNorms
spread.  `pytest -s` prints err, e32 and err / e32 of every result.

Worst err / e32 per group, measured on an MI355X with the fp16-pair library over all layouts of the group's cases (the bound is 8 in
fp32 mode and 64 in f16x3, plus 1e-6 scale; e32 is 1.5e-6 .. 3.6e-6 on the plain and up to 6.5e-6 on the trained-like weights):

    group    weights       fp32   f16x3
    lengths  plain         2.89    5.11      (5 prompts of 31 positions, ragged; the mixed batch, ragged)
    lengths  trained-like  2.33    2.88
    narrow   plain         2.97    5.18      (S = 1; the one-row prompt inside a batch, full length)
    narrow   trained-like  4.57    5.25      (the one-row prompt inside a batch)
    argmax   plain         2.28    4.25
    argmax   trained-like  3.38    2.73
    routes   plain         2.52    5.33      (256 ragged rows; B = 5 at S = 64)
    routes   trained-like  2.90    3.09      (1 ragged row; 129 ragged rows)
    dedup    plain         2.03    3.66
    dedup    trained-like  2.02    2.40

With the bf16-pair library (LADIFF_TEST_LIB=ladiff_amd/libladiff_hip_bf16.so; the split bound is 2048 e32) the worst split-mode ratio is
45.7 (S = 33, trained-like, ragged); per group 22.3 / 45.7 / 33.4 / 33.2 / 20.9; the fp32-mode ratios are those above.  dedup=True
against dedup=False: the same bits in the ragged and full-length layouts, 1.4 e32 apart in the padded one (the launch's L differs).

The oracle of all 53 cases on both weight sets takes 28 s of CPU in total on the MI355X machine (16 threads); the largest case (8193 ragged
rows = 133 prompts x 77 positions on the oracle's side) about 1 s, its whole test 1.6 s.

Against the library of the commit before this file every case passed, with the ratios above: no defect found.  A trial
library with two deliberate faults failed 160 of this file's 213 tests: clip_eos_kernel taking the LAST maximum fails every padded or full-length
case that has a second maximum (EOS padding included) inside L; pooling the ragged layout one row early above 64 prompts fails exactly
the ragged cases of more than 64 prompts (4095 rows and up), while those of up to 1281 rows pass.
"""
import pytest
import torch

from ladiff_amd.text_encoder import MldTextEncoder
from test_gpu_trained_like import check, oracle

import clip_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = ["fp32", "f16x3"]
KINDS = ["plain", "trained"]

_ENC = {}


def encoder(kind, precision):
    if kind not in _ENC:
        m = MldTextEncoder(vocab_size=cc.VOCAB, num_layers=cc.LAYERS)
        m.text_model.load_state_dict(cc.weights(kind), strict=True)
        _ENC[kind] = m.to(DEV).eval()
    m = _ENC[kind]
    m.precision = precision
    return m


def encode_case(name, kind, precision):
    c = cc.CASES[name]
    (want,), (e32,) = oracle(("clip-shapes", kind, name), cc.features_fn(c.ids), cc.weights(kind))
    enc = encoder(kind, precision)
    out = {}
    for layout in c.layouts:
        got = enc.encode_ids(c.ids, dedup=c.dedup, **cc.LAYOUT_KW[layout])
        again = enc.encode_ids(c.ids, dedup=c.dedup, **cc.LAYOUT_KW[layout])
        torch.cuda.synchronize()
        assert got.shape == (c.ids.shape[0], 768) and torch.equal(got, again), (name, layout)
        check(f"CLIP {c.group} | {name} B={c.ids.shape[0]} S={c.ids.shape[1]} rows={cc.rows(c, layout)} {layout} {kind}", precision, got,
              want, e32)
        out[layout] = got
    return c, enc, out, want, e32


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", cc.names("lengths"))
def test_lengths(name, kind, precision):
    """S = 77.  One batch of 2 (the empty prompt), 3, 17, 31 .. 34, 63 .. 66, 76 and 77 positions; 5 prompts of 2 / 31 / 32 / 33 / 64 / 65 /
    77 positions each, where the launch's L itself sits on the edge (one-wave split attention at L <= 32, key words of 32)."""
    encode_case(name, kind, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", cc.names("narrow"))
def test_one_row_prompts_and_narrow_ids(name, kind, precision):
    """A row of equal ids (argmax 0, one row, L = 1) alone and inside a batch; ids of 1, 2 and 33 columns (row stride != 77)."""
    encode_case(name, kind, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", cc.names("argmax"))
def test_argmax_semantics(name, kind, precision):
    """The pooled row is the FIRST position of the LARGEST id: a maximum that is not vocab - 1, one that occurs twice (5 and 69; 67 and 70),
    one at a position >= 64 (the second trip of clip_eos_kernel's lane loop); found on the host (ragged) and on the device (padded, full)."""
    encode_case(name, kind, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", cc.names("routes"))
def test_routes_by_row_count(name, kind, precision):
    """dedup=False.  Ragged totals 256 / 257, 1280 / 1281, 4095 / 4096 / 4097, 5376 / 5377, 8192 / 8193 and 1, 63 / 64 / 65, 128 / 129;
    S = 64 at full length with B = 4 / 5, 20 / 21, 64 / 65, 84 / 85, 128 / 129 (the same edges, and one prompt more); 1, 3, 4, 5, 63, 64
    and 65 short prompts (four rows per workgroup of the row kernels, 64-row tiles of the final projection).  The last row of every
    launch is a pooled row."""
    encode_case(name, kind, precision)


def test_more_than_77_columns_raise():
    """Refused on the host before anything is queued (the tower stays on the CPU here)."""
    enc = MldTextEncoder(vocab_size=cc.VOCAB, num_layers=cc.LAYERS)
    for shape in [(1, 78), (2, 0), (77,)]:
        with pytest.raises(ValueError):
            enc.encode_ids(torch.zeros(shape, dtype=torch.int64))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
def test_dedup_reorders_and_gathers_back(kind, precision):
    """[""] * 3, a, b, a, c, "", b: np.unique sorts the four distinct prompts into another order; rows of identical prompts come back
    bit-identical, and dedup=False gives the same features within the bound."""
    c, enc, out, want, e32 = encode_case("guidance", kind, precision)
    for layout, got in out.items():
        for same in cc.DEDUP_SAME:
            assert all(torch.equal(got[i], got[same[0]]) for i in same), (layout, same)
        plain = enc.encode_ids(c.ids, dedup=False, **cc.LAYOUT_KW[layout])
        check(f"CLIP dedup | guidance {layout} {kind} dedup=False", precision, plain, want, e32)
        check(f"CLIP dedup | guidance {layout} {kind} dedup=True against dedup=False", precision, got, plain.double().cpu(), e32)
