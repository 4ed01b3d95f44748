"""LADiffVae.encode against the fp64 oracle over the shapes and routes that decide which code runs (csrc/encoder.hip, its row
kernels in csrc/rowops.hip, the GEMM routes of csrc/gemm.hip / gemm_big.hip, the attention forms of csrc/attention.hip).

The sequence is [T mu tokens | T logvar tokens | F frames] per sample: S = 2T + F <= 224 rows, M = B S rows per batch.
* GEMM routes by M: fp32 mode moves from the staged kernels to gemm_big at M >= 4096 (the skel-embedding GEMM at B F >= 4096, K = 288
  for nfeats 263, 256 for 251); split mode is gemm_big_split throughout, 64-row tiles, 128-row tiles where ceil(M / 128) (N / 128) > 256
  (M > 4096 for lin1, M > 5376 for in_proj, M > 16384 for the N = 256 products) and at M <= 64.
* the key map is 32-bit words over the S positions: a frame boundary sits on a word boundary at 2T + len = 32, 64, ..., 224.
* the split attention has a one-wave form for S <= 32.
* S < 8: the key map's 8 words have fewer than 8 rows to write them.

Every case: counts, mu / std / latent on ALL rows (mu / std at and behind a sample's count are read by the KL loss) within
trained_like.bound (fp32: 8 e32 + 1e-6 scale; split mode 8 x (fp16 pairs) / 256 x (bf16 pairs) the e32 term; e32 = the oracle's own
fp32-vs-fp64 difference of the case), latent rows >= count exactly zero, a second call the same bits.  Both weight sets: on the plain
synthetic ones one wrongly admitted key moves every sample by > 10 x the f16x3 bound (tests/test_encoder_cases.py), on the trained-like
ones softmax is peaked and the LayerNorms spread.  `pytest -s` prints err, e32 and err / e32 of every result.

Worst err / e32 per group, measured on an MI355X with the fp16-pair library (mu, std and latent together; the bound is 8 in fp32 mode
and 64 in f16x3, plus 1e-6 scale):

    group    weights       fp32   f16x3
    lengths  plain         3.90    7.94      (S = 33, one sample)
    lengths  trained-like  6.15    6.58      (fp32: latent of the latent-count batch, 1.6e-3 against a bound of 2.1e-3)
    MAX_IT   plain         2.84    6.00
    MAX_IT   trained-like  2.74    5.74
    tiny     plain         2.51    8.07      (S = 3 .. 8)
    tiny     trained-like  5.03    6.56
    routes   plain         2.60    7.73      (B = 19 .. 32)
    routes   trained-like  3.41    4.66      (B = 19 .. 80, the DVAE case included)

Against the library of the commit before this file, the 24 cases of S = 3, 5 and 7 (T = 1 with 1 / 3 / 5 frames, T = 2 with 1 / 3, T = 3 with
1 frame; both weight sets, both precisions) failed with LADIFF_ERR_SHAPE from launch_encoder_assemble; every other case passed with the
ratios above.
"""
from types import SimpleNamespace

import pytest
import torch

from ladiff_amd import LADiffVae
from ladiff_amd.schema import ABL, VAE_KW
from oracle import ladiff_oracle as orc
from test_gpu_trained_like import check, oracle

import encoder_cases as ec
import vae_stage_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = ["fp32", "f16x3"]
KINDS = ["plain", "trained"]
NFEATS = [263, 251]

_VAE = {}


def make_vae(kind, nfeats, T, fpl):
    key = (kind, nfeats, T, fpl)
    if key not in _VAE:
        abl = SimpleNamespace(**{**vars(ABL), "MAX_IT": T, "FRAME_PER_LATENT": fpl})
        m = LADiffVae(abl, **{**VAE_KW, "nfeats": nfeats})
        m.load_state_dict(ec.weights(kind, nfeats, T), strict=True)
        _VAE[key] = m.to(DEV).eval()
    m = _VAE[key]
    m.precision = "fp32"
    return m


def encode_case(group, c, kind, precision, corrupt=None):
    x, e = ec.features(c), ec.eps(c)
    x_ref = x if corrupt is None else torch.from_numpy(vae_stage_ref.corrupt(x, *corrupt))
    want, e32 = oracle(("enc-shapes", kind, c), ec.encode_fn(c, x_ref, e), ec.weights(kind, c.nfeats, c.T))
    v = make_vae(kind, c.nfeats, c.T, c.fpl)
    v.precision = precision
    try:
        kw = {} if corrupt is None else {"corrupt": (corrupt[0], corrupt[1].to(DEV))}
        latent, dist, counts = v.encode(x.to(DEV), list(c.lens), eps=e.to(DEV), **kw)
        again = v.encode(x.to(DEV), list(c.lens), eps=e.to(DEV), **kw)
        torch.cuda.synchronize()
    finally:
        v.precision = "fp32"
    assert counts.tolist() == orc.max_iter_elements(c.lens, c.fpl)
    assert latent.shape == (c.T, len(c.lens), 256)
    for i, n in enumerate(counts.tolist()):
        if n < c.T:
            assert latent[n:, i].abs().max().item() == 0, (c.name, i)
    assert torch.equal(latent, again[0]) and torch.equal(dist.loc, again[1].loc) and torch.equal(dist.scale, again[1].scale), c.name
    tag = f"{group} | {c.name} C={c.nfeats} T={c.T} B={len(c.lens)} S={2 * c.T + c.F} {kind}"
    for what, got, w, e_ in zip(("mu", "std", "latent"), (dist.loc, dist.scale, latent), want, e32):
        check(f"encoder {tag} {what}", precision, got, w, e_)


# ---------------------------------------------------------------- lengths: key-map words, latent counts, attention forms, tile edges
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nfeats", NFEATS)
@pytest.mark.parametrize("name", [n for n, _ in ec.LENGTH_EDGES] + [ec.OVER_PADDED[0]])
def test_length_edges(name, nfeats, kind, precision):
    """T = 5: length 1, S = 224, on and beside every latent-count and every key-map word boundary, S = 32 / 33 (one-wave split
    attention), M = 64 / 65; and a tensor longer than its longest sample whose masked frames hold values of size 50."""
    c = next(c for c in ec.length_cases(nfeats) if c.name == name)
    encode_case("lengths", c, kind, precision)


def test_longer_than_the_key_map_raises():
    """F + 2T = 225: refused on the host, before anything is queued."""
    v = make_vae("plain", 263, 5, 48)
    with pytest.raises(NotImplementedError):
        v.encode(torch.zeros(1, 215, 263, device=DEV), [215])


# ---------------------------------------------------------------- MAX_IT other than 5
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,fpl", ec.MAX_IT)
def test_max_it(T, fpl, kind, precision):
    encode_case("MAX_IT", ec.case("lens9", ec.LENS9, T=T, fpl=fpl), kind, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,lens", ec.TINY, ids=[f"T{T}-F{l[0]}" for T, l in ec.TINY])
def test_sequences_of_at_most_8_rows(T, lens, kind, precision):
    """S = 2T + F = 3 .. 8: the key map's 8 words are written although the sample has fewer than 8 rows."""
    encode_case("tiny", ec.case("tiny", lens, T=T, fpl=ec.FPL[T]), kind, precision)


# ---------------------------------------------------------------- GEMM routes by row count
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nfeats", NFEATS)
@pytest.mark.parametrize("B", [19, 20, 21, 26, 27, 32])
def test_routes_by_row_count(B, nfeats, kind, precision):
    """S = 206.  B = 19 / 20 / 21: M = 3914 / 4120 / 4326, B F = 3724 / 3920 / 4116 (fp32: gemm_big from M >= 4096, the skel-embedding
    GEMM on its own at B F >= 4096; split: lin1 on 128-row tiles from M > 4096).  B = 26 / 27: M = 5356 / 5562 (split in_proj,
    M > 5376).  B = 32: an evaluation batch."""
    encode_case("routes", ec.case(f"B{B}", ec.cycled(B), nfeats), kind, precision)


@pytest.mark.parametrize("B", [79, 80])
def test_split_routes_past_16384_rows(B):
    """M = 16274 / 16480: the N = 256 products of the split mode change to 128-row tiles at M > 16384."""
    encode_case("routes", ec.case(f"B{B}", ec.cycled(B)), "trained", "f16x3")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_dvae_on_the_large_route(precision):
    """B = 20 (M = 4120) through `corrupt`: the four corners of the [F, C] block and a seeded 10 % of its positions."""
    c = ec.case("B20_dvae", ec.cycled(20), seed=1)
    F, C = c.F, c.nfeats
    g = torch.Generator().manual_seed(11)
    corners = torch.tensor([0, C - 1, (F - 1) * C, F * C - 1])
    positions = torch.unique(torch.cat([corners, torch.randperm(F * C, generator=g)[:F * C // 10]]))
    values = torch.randn(len(c.lens), positions.numel(), generator=g)
    encode_case("routes", c, "trained", precision, corrupt=(positions, values))
