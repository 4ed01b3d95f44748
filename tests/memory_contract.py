"""The memory contract of a workspace-taking entry, checked from outside.  TEST INFRASTRUCTURE ONLY (a plain helper module).

include/ladiff_hip.h promises: scratch comes from the caller's workspace, sized by the matching `*_workspace_bytes` query; outputs are the
caller's buffers; no result depends on what the workspace or the outputs held before the call.  `run_in_guards` runs a call with its
workspace and every output INSIDE larger int32 buffers (a guard zone of GUARD words on both sides) that are filled - guards, workspace and
outputs alike - with one fill word, and reports what the call returned, how many guard words changed (and the nearest one) and, for a
strided output, how many gap words (columns cols <= j < ld of a row) changed.  `assert_contract` holds the results of the three fills
against each other and against a reference:

    zero       0x00000000   the baseline
    quiet NaN  0x7fc12345   (last bit 1; the canary of scripts/decode_guard.py) any read that reaches a sum, a max or a LayerNorm statistic
    +inf       0x7f800000   (last bit 0) reads a NaN-ignoring max swallows; a tagged hand-off slot nobody primed (parity 0 is what the first
                            use of a slot expects)

A word the call leaves unwritten keeps the fill, so the outputs of the three fills differ (and the NaN / inf ones are not finite); a word of
the workspace that is read before it is written moves the result with the fill; a write outside lands in a guard or a gap.  Nothing here
can fault: an overrun of up to GUARD words is memory the test owns.

`device` makes the helper usable on the CPU (tests/test_memory_contract.py runs it against deliberately wrong torch "entries").
"""
import torch

FILLS = {"zero": 0x00000000, "nan": 0x7fc12345, "inf": 0x7f800000}
GUARD = 1 << 20            # words per side (4 MiB): a wilder write than that no guard catches, and small guards keep the tests quick
ALIGN = 64                 # words: the pointers handed to the entry are 256-byte aligned


class Out:
    """Description of one output buffer: `rows` rows of `cols` words with row stride `ld` (ld == cols: dense), as `dtype` (4-byte)."""

    def __init__(self, rows, cols=1, ld=None, dtype=torch.float32):
        self.rows, self.cols, self.ld, self.dtype = int(rows), int(cols), int(cols if ld is None else ld), dtype
        assert self.ld >= self.cols and torch.empty(0, dtype=dtype).element_size() == 4

    @property
    def words(self):               # from the first word to the last one written: the last row has no gap behind it
        return 0 if self.rows == 0 else (self.rows - 1) * self.ld + self.cols


def _round_up(n, m):
    return (n + m - 1) // m * m


class _Guarded:
    def __init__(self, words, fill, device):
        self.words = int(words)
        self.lo = _round_up(GUARD, ALIGN)
        self.buf = torch.full((self.lo + self.words + GUARD,), _signed(fill), dtype=torch.int32, device=device)
        assert (self.buf.data_ptr() + 4 * self.lo) % (4 * ALIGN) == 0 or self.buf.device.type == "cpu"
        self.fill = _signed(fill)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lo

    @property
    def body(self):
        return self.buf[self.lo:self.lo + self.words]

    def guard_report(self):
        """(guard words that changed, signed distance in words of the nearest one from the body: < 0 below, > 0 above; 0 = none)."""
        below = (self.buf[:self.lo] != self.fill).nonzero().flatten()
        above = (self.buf[self.lo + self.words:] != self.fill).nonzero().flatten()
        n = int(below.numel() + above.numel())
        near = 0
        if above.numel():
            near = int(above.min()) + 1
        if below.numel() and (near == 0 or self.lo - int(below.max()) < near):
            near = -(self.lo - int(below.max()))
        return n, near


def _signed(word):
    return word - (1 << 32) if word >= (1 << 31) else word


def run_in_guards(call, ws_bytes, outputs, fill, device="cuda:0", ws_extra_bytes=0):
    """call(ws_ptr, ws_bytes, out_ptrs) -> return code, run once with the workspace (exactly `ws_bytes`, or `ws_bytes + ws_extra_bytes`
    when a larger workspace is what is being tested) and one buffer per entry of `outputs` ({name: Out}) inside guards, everything filled
    with `fill`.  Returns {"rc", "outputs": {name: tensor [rows, cols] of the Out's dtype, on the CPU}, "guards": {name: (count, nearest)}
    (the workspace under "workspace"), "gaps": {name: changed gap words}}."""
    is_cuda = torch.device(device).type == "cuda"
    given = int(ws_bytes) + int(ws_extra_bytes)
    ws = _Guarded((given + 3) // 4, fill, device)
    bufs = {name: _Guarded(o.words, fill, device) for name, o in outputs.items()}
    if is_cuda:
        torch.cuda.synchronize()
    rc = call(ws.ptr if is_cuda else ws.body, given, {n: (b.ptr if is_cuda else b.body) for n, b in bufs.items()})
    if is_cuda:
        torch.cuda.synchronize()
    res = {"rc": rc, "outputs": {}, "guards": {"workspace": ws.guard_report()}, "gaps": {}, "fill": fill}
    for name, o in outputs.items():
        b = bufs[name]
        res["guards"][name] = b.guard_report()
        body = b.body.cpu()
        if o.rows == 0:
            res["outputs"][name], res["gaps"][name] = body.view(o.dtype).reshape(0, o.cols), 0
            continue
        padded = torch.full((o.rows * o.ld,), b.fill, dtype=torch.int32)
        padded[:o.words] = body
        padded = padded.view(o.rows, o.ld)
        res["gaps"][name] = int((padded[:, o.cols:] != b.fill).sum())
        res["outputs"][name] = padded[:, :o.cols].contiguous().view(o.dtype)
    return res


def run_fills(call, ws_bytes, outputs, device="cuda:0", ws_extra_bytes=0):
    """The zero fill twice (is the entry deterministic at all?), then the NaN and the +inf fill: {"zero", "zero2", "nan", "inf"}."""
    out = {}
    for key, fill in (("zero", "zero"), ("zero2", "zero"), ("nan", "nan"), ("inf", "inf")):
        out[key] = run_in_guards(call, ws_bytes, outputs, FILLS[fill], device, ws_extra_bytes)
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def assert_contract(results_by_fill, want, tol, what):
    """results_by_fill = run_fills(...); want = {name: reference tensor} and tol = {name: absolute bound} (or one number) for the outputs
    that have a reference - the others are still held to guards, gaps, bit identity and finiteness (float outputs).
    Every run returned 0; every guard and gap count is 0; the outputs are bit-identical under the three fills, finite, and within tol of
    want.  An entry whose two zero-fill runs already differ is not deterministic: for it (and only for it) bit identity falls back to
    "every fill within tol", and the returned report says so ("deterministic": False), as does any failure
    message.  The report also carries the guard and gap words counted over all runs and whether the fills gave identical bits."""
    fails = []
    guards = gaps = 0
    for key, r in results_by_fill.items():
        if r["rc"] != 0:
            fails.append(f"{key} fill: the entry returned {r['rc']}")
        guards += sum(n for n, _ in r["guards"].values())
        gaps += sum(r["gaps"].values())
        for name, (n, near) in r["guards"].items():
            if n:
                fails.append(f"{key} fill: {n} guard words of `{name}` changed, the nearest {abs(near)} words {'below' if near < 0 else 'above'} it")
        for name, n in r["gaps"].items():
            if n:
                fails.append(f"{key} fill: {n} gap words (columns cols <= j < ld) of `{name}` changed")
    base = results_by_fill["zero"]["outputs"]
    deterministic = all(torch.equal(_bits(base[n]), _bits(results_by_fill["zero2"]["outputs"][n])) for n in base)
    report = {"guards": guards, "gaps": gaps, "identical": True, "deterministic": deterministic}
    for name in base:
        same = all(torch.equal(_bits(base[name]), _bits(results_by_fill[k]["outputs"][name])) for k in ("nan", "inf"))
        if not same:
            report["identical"] = False
            if deterministic:
                k = next(k for k in ("nan", "inf") if not torch.equal(_bits(base[name]), _bits(results_by_fill[k]["outputs"][name])))
                diff = (_bits(base[name]) != _bits(results_by_fill[k]["outputs"][name]))
                where = diff.nonzero()[0].tolist()
                fails.append(f"`{name}` depends on what the buffers held before the call: {int(diff.sum())} words differ between the zero and "
                             f"the {k} fill, the first at {where} ({base[name][tuple(where)].item()!r} against "
                             f"{results_by_fill[k]['outputs'][name][tuple(where)].item()!r})")
            # not deterministic: the tolerance check below is what holds every fill
    tol_of = (lambda n: tol[n]) if isinstance(tol, dict) else (lambda n: tol)
    for key, r in results_by_fill.items():
        for name, got in r["outputs"].items():
            if got.dtype.is_floating_point and not torch.isfinite(got).all():
                bad = (~torch.isfinite(got)).nonzero()
                fails.append(f"{key} fill: `{name}` has {bad.shape[0]} non-finite words, the first at {bad[0].tolist()}")
            elif name in want:
                w = want[name].reshape(got.shape)
                err = (got.double() - w.double()).abs().max().item() if got.numel() else 0.0
                if not err < tol_of(name):
                    fails.append(f"{key} fill: `{name}` is {err:.3e} from the reference (bound {tol_of(name):.3e})")
    note = ""
    if not deterministic:
        note = " [NOT DETERMINISTIC: two zero-fill runs differ, so the fills were held to the tolerance, not to bit identity]"
        print(f"{what}:{note}")
    assert not fails, f"{what}{note}: " + "; ".join(fails[:8])
    return report


def assert_refused(result, what, code=-3):
    """A call with a workspace below the query: refused on the host (LADIFF_ERR_WORKSPACE) with every output and guard word untouched."""
    assert result["rc"] == code, f"{what}: returned {result['rc']}, expected {code}"
    fill = _signed(result["fill"])
    for name, (n, _) in result["guards"].items():
        assert n == 0, f"{what}: {n} guard words of `{name}` changed by a refused call"
    for name, got in result["outputs"].items():
        assert bool((_bits(got) == fill).all()) and result["gaps"][name] == 0, f"{what}: `{name}` was touched by a refused call"
