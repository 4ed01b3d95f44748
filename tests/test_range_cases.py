"""The range cases do what they claim (CPU; the oracle is the instrument): every case of tests/range_cases.py feeds a matrix product an
operand beyond 131008 - where an fp16 pair is clipped - and its bf16-pair bound is small enough for the GPU comparison
(tests/test_gpu_range.py) to see a clipped operand.  Prints each case's largest operand and bound / scale (`pytest -s`)."""
import pytest
import torch

import range_cases as rc
from test_operand_range import _record
from trained_like import bound


@pytest.mark.parametrize("name", rc.NAMES)
def test_range_case_leaves_fp16_range_and_keeps_a_tight_bound(name):
    c = rc.BY_NAME[name]
    fn, sd = rc.oracle_fn(c), rc.weights(c)
    seen = _record(lambda: fn(torch.float32, sd))
    largest = max(seen["x"], seen["attn"])            # inputs and outputs (q | k | v, hidden) of every `linear`: the products' operands
    want, e32 = rc.oracle(c)
    assert all(torch.isfinite(w).all() for w in want), name
    ratios = []
    for w, e in zip(want, e32):
        scale = max(1.0, w.abs().max().item())
        ratios.append(bound(e, w, "f16x3", 0) / scale)
    print(f"\n[range case] {name}: largest operand {largest:.3e} (GEMM input {seen['x']:.3e}, output {seen['attn']:.3e}, weight "
          f"{seen['w']:.2f}), e32 {max(e32):.3e}, bf16-pair bound / scale {max(ratios):.2e}")
    assert largest > rc.F16_PAIR_MAX, (name, seen)
    assert max(ratios) <= rc.BOUND_CAP, (name, ratios)


def test_clipping_moves_a_case_beyond_its_bound():
    """What the cap is for: the decode case evaluated by the oracle with its latents clipped at +-131008 (what the fp16-pair library does
    to them) differs from the true result by more than the bf16-pair bound."""
    c = rc.BY_NAME["decode_1e5"]
    (want,), (e32,) = rc.oracle(c)
    inp = rc.inputs(c)
    clipped = dict(inp, z=inp["z"].clamp(-rc.F16_PAIR_MAX, rc.F16_PAIR_MAX))
    with torch.no_grad():
        got = rc.oracle_fn(c, clipped)(torch.float64, {k: v.double() for k, v in rc.weights(c).items()})
    err, b = (got - want).abs().max().item(), bound(e32, want, "f16x3", 0)
    print(f"\n[range case] decode_1e5 with latents clipped at 131008: err {err:.3e} against bound {b:.3e}")
    assert err > 10 * b, (err, b)
