"""Model-level cases whose matrix-product operands leave fp16's range.  TEST INFRASTRUCTURE ONLY (a plain helper module, like
encoder_cases.py): shared by tests/test_range_cases.py (CPU: the cases do what they claim) and tests/test_gpu_range.py (GPU against the
fp64 oracle).

The fp16-pair library clips a split operand beyond 131008 (two saturated halves) without any signal; libladiff_hip_bf16.so (bf16 pairs,
fp32's exponent range) is the project's answer for such activations.  A case = one entry of the package fed inputs scaled by `scale`
(1e5 or 1e8): the first matrix product of the entry then reads operands of 3e5 and more, and the LayerNorm that follows it brings the
stream back to O(1), so the oracle's own fp32-vs-fp64 error stays ~1e-5 of the output scale and `trained_like.bound` stays far below
the damage a clipped operand does.  The two conditions every case has to meet (tests/test_range_cases.py asserts them on the CPU):

* the largest matrix-product operand, recorded from the oracle with test_operand_range._record, exceeds F16_PAIR_MAX = 131008;
* trained_like.bound(e32, want, "f16x3", 0) <= 1e-2 max(1, max |want|): above that the comparison could not see a clipped operand.

Cases:  decode of lengths [60, 33, 1] with latents x 1e5 and x 1e8, on the synthetic and on the trained-like decoder weights; the
denoiser forward B = 7, T = 3, masked, t = 481 with the sample, the text, and both x 1e5 (synthetic weights), both x 1e5 on the
trained-like weights, and a text sequence of N = 4 tokens (csrc/linear_ca.hip) with both x 1e5; the LA-VAE encode of the
`vae_encode_humanml` golden with features x 1e5.  Every candidate met both conditions; none was left out.

What each entry's case reaches on the GPU: the denoiser and the encoder convert the scaled input to split operands themselves, so a
conversion that clipped would move them by O(1).  The decoder projects its memory (the latents) to K | V in fp32 in both modes
(csrc/decoder.hip), so the decode cases hold the fp32 side and the kernels behind it to the oracle at that scale, and a clipping split
conversion does not show in them (measured with a trial build: tests/test_gpu_bf16_flavour.py)."""
from collections import namedtuple

import torch

from ladiff_amd import synthetic as syn
from oracle import ladiff_oracle as orc
from conftest import load_golden
from trained_like import oracle_pair, trained_like

F16_PAIR_MAX = 131008.0     # 2 x 65504: beyond it an fp16 pair is clipped
BOUND_CAP = 1e-2            # of max(1, max |want|): a condition on the case, not a tolerance
SEED = 1                    # trained_like's seed, as tests/test_gpu_trained_like.py
DECODE_LENS = [60, 33, 1]

# entry: "decode" | "denoiser" | "encode"; weights: "plain" (ladiff_amd/synthetic.py) | "trained" (trained_like of them);
# scale_x: factor on the latents / the sample / the features; scale_text: factor on the text (denoiser only); n_text: text tokens per prompt
Case = namedtuple("Case", "name entry weights scale_x scale_text n_text")

CASES = [
    Case("decode_1e5", "decode", "plain", 1e5, 1.0, 1),
    Case("decode_1e5_trained", "decode", "trained", 1e5, 1.0, 1),
    Case("decode_1e8", "decode", "plain", 1e8, 1.0, 1),
    Case("decode_1e8_trained", "decode", "trained", 1e8, 1.0, 1),
    Case("denoiser_sample_1e5", "denoiser", "plain", 1e5, 1.0, 1),
    Case("denoiser_text_1e5", "denoiser", "plain", 1.0, 1e5, 1),
    Case("denoiser_both_1e5", "denoiser", "plain", 1e5, 1e5, 1),
    Case("denoiser_both_1e5_trained", "denoiser", "trained", 1e5, 1e5, 1),
    Case("denoiser_both_1e5_ntext4", "denoiser", "plain", 1e5, 1e5, 4),
    Case("encode_1e5", "encode", "plain", 1e5, 1.0, 1),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]

DEN_B, DEN_T, DEN_TIMESTEP = 7, 3, 481

_SD, _ORACLE = {}, {}


def weights(c):
    """The state dict of the case's network (CPU, fp32)."""
    key = ("vae" if c.entry != "denoiser" else "den", c.weights)
    if key not in _SD:
        sd = syn.denoiser_weights() if key[0] == "den" else syn.vae_weights(263)
        _SD[key] = sd if c.weights == "plain" else trained_like(sd, SEED)
    return _SD[key]


def inputs(c):
    """The case's inputs (CPU, fp32), already scaled.  decode: {"z" [5, B, 256], "lens"}; denoiser: {"x" [B, T, 256], "t", "text"
    [B, N, 768], "counts" [B]}; encode: {"features", "lens", "eps"}."""
    if c.entry == "decode":
        z = torch.randn(5, len(DECODE_LENS), 256, generator=torch.Generator().manual_seed(4 + len(DECODE_LENS)))
        for i, l in enumerate(DECODE_LENS):
            z[-(-l // 48):, i] = 0
        return {"z": z * c.scale_x, "lens": list(DECODE_LENS)}
    if c.entry == "denoiser":
        gen = torch.Generator().manual_seed(1000 * DEN_B + 10 * DEN_T + c.n_text)
        x, txt = torch.randn(DEN_B, DEN_T, 256, generator=gen), torch.randn(DEN_B, c.n_text, 768, generator=gen)
        counts = torch.randint(1, DEN_T + 1, (DEN_B,), generator=gen)
        return {"x": x * c.scale_x, "t": DEN_TIMESTEP, "text": txt * c.scale_text, "counts": counts}
    g = load_golden("vae_encode_humanml")
    return {"features": g["features"] * c.scale_x, "lens": g["lengths"].tolist(), "eps": g["eps"]}


def oracle_fn(c, inp=None):
    """fn(dtype, state dict) for trained_like.oracle_pair: the oracle's result(s) of the case."""
    i = inputs(c) if inp is None else inp
    if c.entry == "decode":
        return lambda dt, sd: orc.vae_decode(sd, i["z"].to(dt), i["lens"], frame_per_latent=48)
    if c.entry == "denoiser":
        return lambda dt, sd: orc.denoiser_forward(sd, i["x"].to(dt), i["t"], i["text"].to(dt), i["counts"])
    return lambda dt, sd: orc.vae_encode(sd, i["features"].to(dt), i["lens"], i["eps"].to(dt))


def oracle(c):
    """(fp64 results, e32 per result) of the case, computed once per process and left unchanged."""
    if c.name not in _ORACLE:
        _ORACLE[c.name] = oracle_pair(oracle_fn(c), weights(c))
    return _ORACLE[c.name]
