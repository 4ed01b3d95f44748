"""The memory-contract harness (tests/memory_contract.py) fails on a wrong kernel and passes a correct one - shown on the CPU with torch
"entries", so that nothing has to go wrong on a GPU for the harness to be trusted.

The entry: y[M, N] (row stride ld) = x @ w^T through a workspace that holds the product first, as the HIP entries pass rows through
theirs.  `call(ws, ws_bytes, outs)` gets int32 views (the CPU form of the pointers) of exactly the bytes it may touch - the wrong entries
reach past them through the view's storage, as a kernel with a wrong index would."""
import pytest
import torch

from memory_contract import FILLS, GUARD, Out, assert_contract, assert_refused, run_fills, run_in_guards

M, N, K, LD = 5, 7, 16, 12
X = torch.randn(M, K, generator=torch.Generator().manual_seed(1))
W = torch.randn(N, K, generator=torch.Generator().manual_seed(2))
WANT = {"y": (X.double() @ W.double().t()).float()}
WS_BYTES = M * N * 4
OUTS = {"y": Out(M, N, LD)}


def _beyond(view, words):
    """`words` int32 words starting at the view's first one, whatever the view's own length: the reach of a wrong index."""
    return torch.as_strided(view, (words,), (1,))


def _entry(bug=None):
    def call(ws, ws_bytes, outs):
        if ws_bytes < WS_BYTES:
            return -3
        tmp = _beyond(ws, M * N + 1).view(torch.float32)
        tmp[:M * N] = (X @ W.t()).reshape(-1)
        if bug == "writes_past_workspace":
            tmp[M * N] = 1.0                                       # one word past the end
        y = _beyond(outs["y"], (M - 1) * LD + N).view(torch.float32)
        for r in range(M):
            row = tmp[r * N:(r + 1) * N].clone()
            if bug == "leaves_output_unwritten" and r == M - 1:
                y[r * LD:r * LD + N - 1] = row[:N - 1]              # the last word of the last row is never stored
            else:
                y[r * LD:r * LD + N] = row
        return 0
    return call


def _reads_unwritten():
    """An entry sized for one spare word that it adds into its output without ever writing it."""
    def call(ws, ws_bytes, outs):
        tmp = ws.view(torch.float32)
        tmp[:M * N] = (X @ W.t()).reshape(-1)
        y = _beyond(outs["y"], (M - 1) * LD + N).view(torch.float32)
        for r in range(M):
            row = tmp[r * N:(r + 1) * N].clone()
            if r == 2:
                row[3] = row[3] + tmp[M * N]                        # the spare word: inside the workspace, never written
            y[r * LD:r * LD + N] = row
        return 0
    return call


def test_a_correct_entry_passes():
    rep = assert_contract(run_fills(_entry(), WS_BYTES, OUTS, device="cpu"), WANT, 1e-5, "correct entry")
    assert rep == {"guards": 0, "gaps": 0, "identical": True, "deterministic": True}
    # ... with a larger workspace too, and a short one is refused untouched
    assert_contract(run_fills(_entry(), WS_BYTES, OUTS, device="cpu", ws_extra_bytes=4096), WANT, 1e-5, "correct entry, larger workspace")
    assert_refused(run_in_guards(_entry(), WS_BYTES - 4, OUTS, FILLS["nan"], device="cpu"), "correct entry, short workspace")


def test_a_write_past_the_workspace_is_caught():
    with pytest.raises(AssertionError, match="guard words of `workspace` changed, the nearest 1 words above"):
        assert_contract(run_fills(_entry("writes_past_workspace"), WS_BYTES, OUTS, device="cpu"), WANT, 1e-5, "overrun")


def test_a_read_of_an_unwritten_workspace_word_is_caught():
    res = run_fills(_reads_unwritten(), WS_BYTES + 4, OUTS, device="cpu")
    # under the zero fill alone the entry is right - which is how such a read survives a suite that reuses allocator blocks
    assert (res["zero"]["outputs"]["y"] - WANT["y"]).abs().max().item() < 1e-5
    with pytest.raises(AssertionError, match="depends on what the buffers held before the call"):
        assert_contract(res, WANT, 1e-5, "unwritten read")


def test_an_unwritten_output_word_is_caught():
    res = run_fills(_entry("leaves_output_unwritten"), WS_BYTES, OUTS, device="cpu")
    with pytest.raises(AssertionError, match="depends on what the buffers held before the call"):
        assert_contract(res, WANT, 1e-5, "unwritten output")
    # even with the other fills' outputs made equal, the NaN that stayed in the output is a failure of its own
    with pytest.raises(AssertionError, match="non-finite"):
        assert_contract({k: res["nan"] for k in res}, WANT, 1e-5, "unwritten output, NaN fill only")


def test_a_write_into_the_gap_columns_is_caught():
    def call(ws, ws_bytes, outs):
        rc = _entry()(ws, ws_bytes, outs)
        _beyond(outs["y"], LD).view(torch.float32)[N] = 2.0        # column N of row 0: between the rows
        return rc
    with pytest.raises(AssertionError, match="1 gap words"):
        assert_contract(run_fills(call, WS_BYTES, OUTS, device="cpu"), WANT, 1e-5, "gap write")


def test_a_launch_on_a_short_workspace_is_caught():
    def call(ws, ws_bytes, outs):                                   # no host check: writes its output whatever it was given
        _beyond(outs["y"], N).view(torch.float32)[:] = 0.0
        return 0
    with pytest.raises(AssertionError):
        assert_refused(run_in_guards(call, WS_BYTES - 4, OUTS, FILLS["nan"], device="cpu"), "no host check")
