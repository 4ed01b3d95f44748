"""Operands beyond fp16's range on the GPU (tests/range_cases.py; tests/test_range_cases.py shows on the CPU that every case has one).

What is asserted depends on the loaded library's split format (`ladiff_split_format()`):

* fp32 mode, either library: within trained_like.bound of the fp64 oracle - fp32 has the range.
* split mode, bf16 pairs (libladiff_hip_bf16.so; tests/test_gpu_bf16_flavour.py runs these ids on it in a child process): within
  trained_like.bound(..., split_format=0) of the fp64 oracle, rows past a motion's length exactly zero.  This is what the library exists
  for.
* split mode, fp16 pairs (the product): the result is finite, nothing more - an operand beyond 131008 is clipped there, which is the
  documented behaviour (csrc/common.h; `LADIFF.check_split_range` sends such users to the bf16 library).

Kernel level: `ladiff_gemm_resident` (split) and `ladiff_gemm_split` with A at scale 3e5 and 1e30 (W scaled down, the products stay
finite in fp32) through test_gpu_kernels.assert_three_term_product, whose bound is relative to |A| |W|^T; with bf16 pairs also against
the fp64 product of the UNSPLIT operands (the three-term emulation reads the planes the kernel read: a conversion that clips shows only
against the unsplit ones).  One split self-attention with V at 3e5 and q, k at O(1)."""
import math

import pytest
import torch

from ladiff_amd import LADiffDenoiser, LADiffVae, _lib
from oracle import ladiff_oracle as orc
import range_cases as rc
from test_abi import ABL, DEN_KW, VAE_KW
from test_gpu_kernels import assert_three_term_product, gemm_resident, ref_gemm, rnd, to_split
from trained_like import bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = ["fp32", "f16x3"]


def lib():
    return _lib.lib()


def bf16_pairs():
    return lib().ladiff_split_format() == 0


_MODULES = {}


def module(c):
    key = ("den" if c.entry == "denoiser" else "vae", c.weights)
    if key not in _MODULES:
        m = LADiffDenoiser(ABL, **DEN_KW) if key[0] == "den" else LADiffVae(ABL, **VAE_KW)
        m.load_state_dict(rc.weights(c), strict=True)
        _MODULES[key] = m.to(DEV).eval()
    return _MODULES[key]


def check(name, precision, got, want, e32):
    got = got.detach().double().cpu()
    assert got.shape == want.shape and torch.isfinite(got).all(), name
    if precision != "fp32" and not bf16_pairs():
        print(f"\n[range] {name}, {precision}, fp16 pairs: finite (operands beyond 131008 are clipped: no comparison)")
        return
    err, b = (got - want).abs().max().item(), bound(e32, want, precision, lib().ladiff_split_format())
    print(f"\n[range] {name}, {precision}: err {err:.3e}  e32 {e32:.3e}  err/e32 {err / max(e32, 1e-30):7.2f}  bound {b:.3e}  "
          f"max|want| {want.abs().max().item():.2f}")
    assert err <= b, (name, precision, err, b)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", rc.NAMES)
def test_range_case(name, precision):
    c = rc.BY_NAME[name]
    inp, (want, e32), m = rc.inputs(c), rc.oracle(c), module(c)
    m.precision = precision
    try:
        if c.entry == "decode":
            got = m.decode(inp["z"].to(DEV), inp["lens"])
            torch.cuda.synchronize()
            for i, l in enumerate(inp["lens"]):
                if l < got.shape[1]:
                    assert got[i, l:].abs().max().item() == 0, (name, i)
            results = [("frames", got)]
        elif c.entry == "denoiser":
            got = m(inp["x"].to(DEV), torch.tensor(inp["t"]), inp["text"].to(DEV), max_iter_elements=inp["counts"].to(DEV))[0]
            torch.cuda.synchronize()
            results = [("eps", got)]
        else:
            latent, dist, counts = m.encode(inp["features"].to(DEV), inp["lens"], eps=inp["eps"].to(DEV))
            torch.cuda.synchronize()
            for i, k in enumerate(counts.tolist()):
                if k < latent.shape[0]:
                    assert latent[k:, i].abs().max().item() == 0, (name, i)
            results = [("mu", dist.loc), ("std", dist.scale), ("latent", latent)]
    finally:
        m.precision = "fp32"
    for (what, got), w, e in zip(results, want, e32):
        check(f"{name} {what}", precision, got, w, e)


# ---------------------------------------------------------------- kernel level
# A at 3e5 against W at O(1 / sqrt(K)); A at 1e30 against W scaled down by 1e-10: products of 1e20, finite in fp32 (an fp16 half holds
# neither: there A is clipped and W is zero, and the three-term emulation of the planes says so too)
A_AND_W_SCALES = [(3e5, 1.0), (1e30, 1e-10)]


def against_unsplit_operands(got, A, W, what):
    """bf16 pairs only: 2^-16 per operand, two operands, three terms -> 4 x 2^-16 of (|A| |W|^T) per element (the bound of
    test_gpu_kernels.test_gemm_resident_split, per element instead of its maximum); a clipped operand is off by O(1) of it."""
    assert torch.isfinite(got).all(), what
    if not bf16_pairs():
        return
    mag = A.abs().double() @ W.abs().double().t()
    err = (got.double() - ref_gemm(A, W)).abs()
    worst = (err / (4 * 2.0 ** -16 * mag + 1e-30)).max().item()
    print(f"[range] {what}: max err / (4 x 2^-16 |A||W|^T) = {worst:.3f}")
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize("scale,wscale", A_AND_W_SCALES)
@pytest.mark.parametrize("M,N,K", [(77, 256, 256), (90, 256, 512)])
def test_gemm_resident_split_beyond_fp16(M, N, K, scale, wscale):
    A, W = rnd(M, K, scale=scale), rnd(N, K, scale=wscale / math.sqrt(K), seed=1)
    ops = {}
    planes = gemm_resident(A, W, split=True, keep=ops)
    if K == 256:
        assert_three_term_product(planes, ops["A"], ops["W"], K)
        got = planes
    else:
        for i in range(K // 256):
            assert_three_term_product(planes[i], ops["A"][:, 256 * i:256 * (i + 1)], ops["W"][:, 256 * i:256 * (i + 1)], 256)
        got = planes.double().sum(0)
    against_unsplit_operands(got, A, W, f"gemm_resident split M={M} K={K} A x {scale:g}")


@pytest.mark.parametrize("scale,wscale", A_AND_W_SCALES)
@pytest.mark.parametrize("M,N,K", [(130, 128, 256), (1, 128, 64)])
def test_gemm_split_large_m_beyond_fp16(M, N, K, scale, wscale):
    A, W = rnd(M, K, scale=scale), rnd(N, K, scale=wscale / math.sqrt(K), seed=1)
    As, Ws = to_split(A), to_split(W)
    Y = torch.full((M, N), float("nan"), device=DEV)
    _lib.check(lib().ladiff_gemm_split(_lib.ptr(As), K, None, 0, K, _lib.ptr(Ws), K, None, None, 0, _lib.ptr(Y), None, N, M, N, K,
                                       _lib.ACT["none"], _lib.stream_ptr()))
    torch.cuda.synchronize()
    got = Y.cpu()
    assert_three_term_product(got, As, Ws, K)
    against_unsplit_operands(got, A, W, f"gemm_split M={M} K={K} A x {scale:g}")


def test_self_attention_split_values_beyond_fp16():
    """V at 3e5, q and k at O(1): the kernel converts q | k | v itself.  bf16 pairs: a logit carries 2^-16 relative per operand and per
    half (4 x 2^-16 max |s| in all), which moves every softmax weight by that much relative, and v and the probabilities carry 2^-16
    each: err <= (4 x 2^-16 max |s| + 4 x 2^-16) max |v|.  fp16 pairs clip v: finite only."""
    lengths, nheads = [1, 33, 32, 31, 101], 4
    B, Fr, W = len(lengths), max(lengths), 64 * nheads
    qkv = rnd(B * Fr, 3 * W)
    qkv.view(B * Fr, 3, W)[:, 2] *= 3e5
    out = torch.full((B * Fr, W), float("nan"), device=DEV)
    qd, ld = qkv.to(DEV), torch.tensor(lengths, dtype=torch.int32, device=DEV)
    _lib.check(lib().ladiff_self_attention_split(_lib.ptr(qd), ld.data_ptr(), None, _lib.ptr(out), B, Fr, nheads, 0, _lib.stream_ptr()))
    torch.cuda.synchronize()
    got = out.cpu()
    valid = orc.lengths_to_mask(lengths, Fr).reshape(-1)
    assert torch.isfinite(got[valid]).all()
    if not bf16_pairs():
        return
    q, k, v = qkv.double().view(B, Fr, 3, nheads, 64).permute(2, 0, 3, 1, 4)
    s = ((q * 0.125) @ k.transpose(-1, -2)).masked_fill((~orc.lengths_to_mask(lengths, Fr))[:, None, None, :], float("-inf"))
    want = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B * Fr, W)
    smax = s[torch.isfinite(s)].abs().max().item()
    b = (4 * 2.0 ** -16 * smax + 4 * 2.0 ** -16) * v.abs().max().item()
    err = (got.double() - want)[valid].abs().max().item()
    print(f"\n[range] split self-attention, V x 3e5: err {err:.3e}  bound {b:.3e}  max|s| {smax:.2f}  max|v| {v.abs().max().item():.3e}")
    assert err <= b, (err, b)
