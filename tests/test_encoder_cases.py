"""The encoder's length cases (tests/encoder_cases.py, run on the GPU by tests/test_gpu_encoder_shapes.py) can see the fault they are
meant for.  CPU only: the oracle is the instrument, the library is not loaded.

For every length case on the plain synthetic weights the tensor is padded by one N(0, 1) frame and the fp64 oracle is run again with the
frame-key mask taken from lengths + 1 (the features, the latent counts and the token keys unchanged): every sample then admits exactly one
key it must not see.  Each sample's mu must move by more than 10 x the f16x3 bound of the case's mu (trained_like.bound with fp16 pairs,
the product's default split format).  This is a condition on the INPUTS: a case that misses it gets another seed or other lengths, never
another factor.  `pytest -s` prints the least-moved sample of every case; measured: bounds 1.3e-4 .. 1.8e-4, the least-moved sample at
2.8e-2 (174 x the bound; the batches with samples of ~200 keys) to 4.2 (the masked frames of size 50).

On trained-like weights the least-moved sample lies inside the split bound (peaked softmax: one more key with a small logit weighs
nothing), which is why the GPU file runs both weight sets: synthetic for indexing and masks, trained-like for softmax and LayerNorm."""
import pytest
import torch

from trained_like import bound, oracle_pair

import encoder_cases as ec

FACTOR = 10.0


@pytest.mark.parametrize("nfeats", [263, 251])
@pytest.mark.parametrize("name", [n for n, _ in ec.LENGTH_EDGES] + [ec.OVER_PADDED[0]])
def test_one_wrongly_admitted_key_moves_every_sample(name, nfeats):
    c = next(c for c in ec.length_cases(nfeats) if c.name == name)
    sd = ec.weights("plain", nfeats, c.T)
    x, e = ec.features(c), ec.eps(c)
    (mu, _, _), (e32, _, _) = oracle_pair(ec.encode_fn(c, x, e), sd)
    b = bound(e32, mu, "f16x3", 1)
    extra = torch.randn(len(c.lens), 1, nfeats, generator=torch.Generator().manual_seed(5))
    xp = torch.cat([x, extra], dim=1)
    with torch.no_grad():
        mu1 = ec.encode_fn(c, xp, e, key_lengths=[l + 1 for l in c.lens])(torch.float64, {k: v.double() for k, v in sd.items()})[0]
    moved = (mu1 - mu).abs().amax(dim=(0, 2))                   # per sample, all T rows of mu
    print(f"\n[encoder cases] {name} C={nfeats}: e32 {e32:.2e}  f16x3 bound {b:.2e}  least-moved sample {moved.min().item():.2e} "
          f"= {moved.min().item() / b:.0f} x the bound")
    assert (moved > FACTOR * b).all(), (name, nfeats, moved.tolist(), b)
