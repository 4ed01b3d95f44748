"""The trained-like weight transform of tests/trained_like.py meets its conditions, and the bounds built on it see what the synthetic
weights hide.  CPU only: the oracle (oracle/ladiff_oracle.py) is the instrument, the library is not loaded.

Measured here (`pytest -s tests/test_trained_like.py` prints them; logit std min ... max over the layers | model's largest |logit| |
mean largest probability min ... max over the layers):

    synthetic weights (constructor-like):
      decoder self-attention, 196 keys         std  0.15 ...  0.81 | max   3.2 | largest probability 0.14 ... 0.15
      decoder cross-attention, 5 keys          std  0.45 ...  0.54 | max   2.4 | largest probability 0.68 ... 0.69
      denoiser self-attention, 7 keys          std  0.51 ...  0.97 | max   4.4 | largest probability 0.35 ... 0.42
      denoiser linear cross-attn, 64 columns   std  0.97 ...  1.02 | max   4.5 | largest probability 0.10 ... 0.11
      encoder self-attention, 206 keys         std  0.48 ...  0.70 | max   3.7 | largest probability 0.02 ... 0.04
      CLIP self-attention, 2 layers            std  0.83 ...  0.95 | max   5.4 | largest probability 0.12 ... 0.17
    trained_like(sd, 1):
      decoder self-attention, 196 keys         std  3.09 ... 23.21 | max  68.7 | largest probability 0.28 ... 0.69
      decoder cross-attention, 5 keys          std  9.42 ... 12.49 | max  43.8 | largest probability 0.96 ... 0.97
      denoiser self-attention, 7 keys          std  4.89 ... 15.57 | max  68.9 | largest probability 0.80 ... 0.90
      denoiser linear cross-attn, 64 columns   std  3.33 ...  4.05 | max  16.0 | largest probability 0.44 ... 0.59
      encoder self-attention, 206 keys         std 10.82 ... 18.50 | max  89.3 | largest probability 0.66 ... 0.83
      CLIP self-attention, 2 layers            std 11.24 ... 12.63 | max  59.0 | largest probability 0.80 ... 0.85

Sensitivity (test_perturbed_oracle_exceeds_the_bounds): max |perturbed fp32 oracle - fp64 oracle| against the bounds of
`trained_like.bound`:

    decode,   trained-like (e32 4.6e-5, bound fp32 3.7e-4, f16x3 2.9e-3): probabilities as one fp16 6.4e-3; other norm's gamma / beta 3.4;
                                                                        one-pass variance 5.6e-5 (NOT beyond either bound)
    denoiser, trained-like (e32 1.8e-5, bound fp32 1.5e-4, f16x3 1.2e-3): probabilities as one fp16 2.0e-3; other norm's gamma / beta 4.5;
                                                                        one-pass variance 1.8e-5 (NOT beyond either bound)
    synthetic weights against the existing tolerances (decode 1e-4 fp32 / 5e-4 f16x3, denoiser 5e-5 / 1e-3): probabilities as one fp16
    6.1e-4 / 6.2e-4 - above the fp32 tolerances, at the f16x3 ones (above 5e-4 on the decode, below 1e-3 on the denoiser: the old tests
    catch it in the decoder only by 1.2 x); other norm's gamma / beta 0.10 / 0.16 - the old tests catch it too (kept: here it misses by
    1000 x instead of 100 x); one-pass variance 3.6e-6 - invisible to old and new model-level tests alike.  The residual stream's row
    means are O(1) like its std, and the one-pass form errs by 2^-24 mean^2 / var: it is pinned on rows of mean 1000 / std 1 instead
    (test_one_pass_variance_misses_the_row_bound here: 430 x the derived row bound; tests/test_gpu_kernels.py on the kernels).
"""
import pytest
import torch
import torch.nn.functional as F

from ladiff_amd import synthetic as syn
from oracle import ladiff_oracle as orc
from conftest import load_golden
from trained_like import (LN_EPS, bound, layernorm_row_bound, offset_rows, oracle_pair, softmax_probe, spread_affine, summary,
                          trained_like)

LENS = [196, 60, 120, 1, 77, 48, 150, 33]
F16_MAX = 65504.0
SEED = 1


def _inputs():
    gen = torch.Generator().manual_seed(4)
    z = torch.randn(5, len(LENS), 256, generator=gen)
    for i, l in enumerate(LENS):
        z[-(-l // 48):, i] = 0
    x, txt = torch.randn(12, 5, 256, generator=gen), torch.randn(12, 1, 768, generator=gen)
    counts = torch.randint(1, 6, (12,), generator=gen)
    return z, x, txt, counts


Z, X, TXT, COUNTS = _inputs()


def decode(dt, sd):
    return orc.vae_decode(sd, Z.to(dt), LENS)


def denoise(dt, sd):
    return orc.denoiser_forward(sd, X.to(dt), 981, TXT.to(dt), COUNTS)


def encode(dt, sd):
    g = load_golden("vae_encode_humanml")
    return orc.vae_encode(sd, g["features"].to(dt), g["lengths"].tolist(), g["eps"].to(dt))


def clip(dt, sd):
    return orc.clip_text_features(sd, syn.clip_token_ids(6, 512, empty_first=3), 2, 12)


def weights(trained):
    tr = (lambda s: trained_like(s, SEED)) if trained else (lambda s: s)
    return tr(syn.vae_weights(263)), tr(syn.denoiser_weights()), tr(syn.clip_weights(512, 2))


def probe_all(trained):
    """{softmax family: (std min, std max, largest |logit|, top min, top max)} + the models' outputs."""
    vae, den, cl = weights(trained)
    out_d, c_dec = softmax_probe(lambda: decode(torch.float32, vae))
    out_n, c_den = softmax_probe(lambda: denoise(torch.float32, den))
    out_e, c_enc = softmax_probe(lambda: encode(torch.float32, vae))
    out_c, c_clip = softmax_probe(lambda: clip(torch.float32, cl))
    assert len(c_dec) == 18 and len(c_den) == 27 and len(c_enc) == 9 and len(c_clip) == 2
    assert all(c["keys"] == 196 for c in c_dec[0::2]) and all(c["keys"] == 5 for c in c_dec[1::2])
    stats = {"decoder self-attention, 196 keys": summary(c_dec[0::2]), "decoder cross-attention, 5 keys": summary(c_dec[1::2]),
             "denoiser self-attention, 7 keys": summary(c_den[0::3]), "denoiser linear cross-attn, 64 columns": summary(c_den[1::3]),
             "encoder self-attention, 206 keys": summary(c_enc), "CLIP self-attention, 2 layers": summary(c_clip)}
    per_layer = {"decoder": c_dec[0::2], "denoiser": c_den[0::3], "encoder": c_enc, "clip": c_clip}
    return stats, per_layer, (out_d, out_n, out_e, out_c)


def _print(title, stats):
    print(f"\n{title}")
    for name, (s0, s1, mx, t0, t1) in stats.items():
        print(f"  {name:40s} std {s0:5.2f} ... {s1:5.2f} | max {mx:6.1f} | largest probability {t0:.2f} ... {t1:.2f}")


def test_trained_like_is_deterministic_and_keeps_the_schema():
    sd = syn.vae_weights(263)
    a, b, c = trained_like(sd, 3), trained_like(dict(reversed(list(sd.items()))), 3), trained_like(sd, 4)
    assert list(a) == list(sd) and all(torch.equal(a[k], b[k]) for k in sd)                # order of the keys does not matter
    assert not torch.equal(a["decoder.norm.weight"], c["decoder.norm.weight"])
    blk = "decoder.middle_block."
    # each LayerNorm has its own draw: no two norms of a layer share gamma or beta, and gamma is spread
    for kind in ("weight", "bias"):
        n1, n2, n3 = (a[f"{blk}norm{i}.{kind}"] for i in (1, 2, 3))
        assert (n1 - n2).abs().max() > 0.5 and (n2 - n3).abs().max() > 0.5 and (n1 - n3).abs().max() > 0.5
    g = a[blk + "norm1.weight"]
    assert g.min() > 0 and g.max() / g.median() > 2.5
    # matrices other than the q | k projections are untouched; the v rows too
    assert torch.equal(a[blk + "linear1.weight"], sd[blk + "linear1.weight"])
    assert torch.equal(a[blk + "self_attn.in_proj_weight"][512:], sd[blk + "self_attn.in_proj_weight"][512:])
    assert torch.equal(a[blk + "self_attn.in_proj_weight"][:512], sd[blk + "self_attn.in_proj_weight"][:512] * 4.2)
    # far inside the fp16 halves' range: the checkpoint loader's split-range check passes on these weights
    for sd_t in weights(True):
        assert max(v.abs().max().item() for v in sd_t.values()) < F16_MAX / 1024
        assert all(torch.isfinite(v).all() for v in sd_t.values())


def test_synthetic_softmaxes_are_flat():
    """The reason for this file: on the untransformed synthetic weights no logit of any model reaches 6."""
    stats, _, _ = probe_all(False)
    _print("synthetic weights", stats)
    assert max(s[2] for s in stats.values()) < 6
    assert stats["decoder self-attention, 196 keys"][4] < 0.2


@pytest.fixture(scope="module")
def trained_probe():
    return probe_all(True)


def test_trained_like_softmaxes_are_peaked(trained_probe):
    stats, per_layer, outs = trained_probe
    _print("trained-like weights", stats)
    for model, calls in per_layer.items():
        assert all(c["std"] >= 2 for c in calls), (model, [c["std"] for c in calls])
        assert 20 <= max(c["max"] for c in calls) <= 100, (model, max(c["max"] for c in calls))
    assert all(c["top"] >= 0.25 for c in per_layer["decoder"]), [c["top"] for c in per_layer["decoder"]]
    flat = [t for o in outs for t in (o if isinstance(o, tuple) else (o,))]
    assert all(torch.isfinite(t).all() for t in flat)
    assert outs[0].abs().max().item() < 100


def test_oracle_fp32_error_keeps_the_bounds_meaningful():
    vae, den, _ = weights(True)
    (_,), (e_dec,) = oracle_pair(decode, vae)
    (_,), (e_den,) = oracle_pair(denoise, den)
    (_,), (s_dec,) = oracle_pair(decode, syn.vae_weights(263))
    print(f"\ne32 = max |oracle fp32 - oracle fp64|: decode {e_dec:.2e} (synthetic {s_dec:.2e}), denoiser {e_den:.2e}")
    assert e_dec <= 2e-4 and e_den <= 2e-4


# ---------------------------------------------------------------- sensitivity: three ways a kernel could be wrong, applied to the oracle
class _Patched:
    def __init__(self, obj, name, new):
        self.obj, self.name, self.new = obj, name, new

    def __enter__(self):
        self.old = getattr(self.obj, self.name)
        setattr(self.obj, self.name, self.new)

    def __exit__(self, *a):
        setattr(self.obj, self.name, self.old)


def _softmax_fp16_probabilities():
    """The probabilities rounded to ONE fp16 (the lo half of the hi + lo pair lost)."""
    real = torch.softmax
    return _Patched(torch, "softmax", lambda x, dim=-1, **kw: real(x, dim=dim, **kw).half().to(x.dtype))


def _one_pass_variance():
    """var = E[x^2] - E[x]^2 in fp32 instead of the two-pass form."""
    def layer_norm(x, w, b):
        xf = x.float()
        mean = xf.mean(-1, keepdim=True)
        var = (xf * xf).mean(-1, keepdim=True) - mean * mean
        return (((xf - mean) * torch.rsqrt(var.clamp_min(0) + orc.EPS_LN)) * w.float() + b.float()).to(x.dtype)
    return _Patched(orc, "layer_norm", layer_norm)


def _other_norm(sd):
    """Every layer's norm1 and norm2 exchange gamma and beta (the parameters of the layer's OTHER LayerNorm)."""
    out = dict(sd)
    for k in sd:
        if ".norm1." in k:
            k2 = k.replace(".norm1.", ".norm2.")
            out[k], out[k2] = sd[k2], sd[k]
    return out


# the loosest assertion the existing model-level tests make on these outputs, per arithmetic mode (tests/test_gpu_path.py:
# test_vae_decode_golden 1e-4, test_vae_decode_golden_split FRAME_TOL / 2; test_denoiser_forward_golden 5e-5, test_denoiser_forward_split 1e-3)
CURRENT_TOL = {"decode": {"fp32": 1e-4, "f16x3": 5e-4}, "denoiser": {"fp32": 5e-5, "f16x3": 1e-3}}


@pytest.mark.parametrize("model", ["decode", "denoiser"])
def test_perturbed_oracle_exceeds_the_bounds(model):
    """Each perturbation of the fp32 oracle, on the trained-like weights, against the fp64 oracle: beyond the bounds the GPU tests hold the
    kernels to (fp32 mode and the f16x3 mode of fp16 pairs).  On the synthetic weights the same perturbations are reported against the
    tolerances of the existing tests."""
    fn = decode if model == "decode" else denoise
    pick = (lambda w: w[0]) if model == "decode" else (lambda w: w[1])
    rows = []
    for trained in (True, False):
        sd = pick(weights(trained))
        (want,), (e32,) = oracle_pair(fn, sd)
        b32, b16 = bound(e32, want, "fp32"), bound(e32, want, "f16x3", 1)
        errs = {}
        with torch.no_grad():
            with _softmax_fp16_probabilities():
                errs["softmax probabilities as one fp16"] = (fn(torch.float32, sd).double() - want).abs().max().item()
            errs["gamma / beta of the layer's other LayerNorm"] = (fn(torch.float32, _other_norm(sd)).double() - want).abs().max().item()
            with _one_pass_variance():
                errs["one-pass fp32 variance"] = (fn(torch.float32, sd).double() - want).abs().max().item()
        rows.append((trained, e32, b32, b16, errs))
        name = "trained-like" if trained else "synthetic"
        print(f"\n{model}, {name} weights: e32 {e32:.2e}, bound fp32 {b32:.2e}, bound f16x3 (fp16 pairs) {b16:.2e}")
        for what, err in errs.items():
            if trained:
                print(f"  {what:45s} {err:.2e} = {err / b32:8.1f} x fp32 bound, {err / b16:8.1f} x f16x3 bound")
            else:
                tol = CURRENT_TOL[model]
                print(f"  {what:45s} {err:.2e}: " + ", ".join(
                    f"{'below' if err < tol[m] else 'ABOVE'} the current {m} tolerance {tol[m]:.0e}" for m in ("fp32", "f16x3")))
    _, e32, b32, b16, errs = rows[0]
    # the one-pass variance is NOT visible at model level on either weight set (measured 0.2 x / 2.6 x the fp32 bound, below the f16x3
    # bound): the residual stream's row means are O(1) like its std, and the one-pass form errs by 2^-24 mean^2 / var.  It is reported
    # here and pinned by the unit-level rows instead (test_one_pass_variance_misses_the_row_bound, tests/test_gpu_kernels.py).
    for what, err in errs.items():
        assert err > b32 or what == "one-pass fp32 variance", (what, err, b32)
    assert errs["softmax probabilities as one fp16"] > b16 and errs["gamma / beta of the layer's other LayerNorm"] > b16, (errs, b16)


def test_one_pass_variance_misses_the_row_bound():
    """The unit-level rows of tests/test_gpu_kernels.py (mean 1000 / std 1, mean -300 / std 0.01, constant, one outlier) with spread
    gamma / beta: a two-pass fp32 LayerNorm on the CPU holds the derived per-row bound, the one-pass form misses it by orders of
    magnitude on the offset rows."""
    x = offset_rows(40)
    gamma, beta = spread_affine(5)
    want = F.layer_norm(x.double(), (256,), gamma.double(), beta.double(), LN_EPS)
    bnd = layernorm_row_bound(x, gamma)
    two = F.layer_norm(x, (256,), gamma, beta, LN_EPS)
    assert ((two.double() - want).abs() <= bnd).all()
    with _one_pass_variance():
        one = orc.layer_norm(x, gamma, beta)
    ratio = ((one.double() - want).abs() / bnd).amax(dim=1)
    print("\none-pass variance, error / row bound by row kind (mean 1000, mean -300, constant, outlier, plain): " +
          ", ".join(f"{ratio[k::5].max().item():.1f}" for k in range(5)))
    assert ratio[0::5].min() > 30 and ratio[1::5].min() > 30
    assert torch.equal(want[2], beta.double()) and torch.equal(two[2], beta)            # constant rows: exactly beta
