"""The evaluator cases (tests/evaluator_cases.py, run on the GPU by tests/test_gpu_evaluator_shapes.py) meet the conditions their bounds
rest on, and can see the mistakes they are meant for.  CPU only: the oracle is the instrument, the library is not loaded.

* Gate regime: on the default cases the trained-like GRUs have at least a tenth of their r / z gate values outside [0.01, 0.99] and at least
  a tenth inside [0.1, 0.9], at the smallest gain of {2, 3, 4, 6, 8} that does; the synthetic ones have none saturated (which is why the
  GPU file runs both).
* e32 (the oracle's own fp32-vs-fp64 difference) of every case is below 1e-4 max(1, max |want|): `trained_like.bound` = 8 e32 + 1e-6 scale
  then stays a statement about fp32 arithmetic.
* Each mutation (a) .. (h) of a local restatement of the oracle moves the fp64 result of at least one listed case by more than
  100 x that case's bound.  These are conditions on the INPUTS: a case that misses one gets other lengths or another seed, never another
  factor.  `pytest -s` prints the figures."""
import pytest
import torch
import torch.nn.functional as F

from oracle import ladiff_oracle as orc
from trained_like import bound, oracle_pair

import evaluator_cases as ev

E32_CAP = 1e-4
SATURATED_SHARE = 0.1          # of the r / z values outside [0.01, 0.99]
OPEN_SHARE = 0.1               # inside [0.1, 0.9]
FACTOR = 100.0


# ---------------------------------------------------------------- the oracle's evaluator functions restated, with one mistake each
def movement(sd, feats, mut=None):
    slope = 0.01 if mut == "e" else 0.2
    x = feats[..., :-4].permute(0, 2, 1)
    for key in ("main.0", "main.3"):
        w = sd[key + ".weight"]
        if mut == "f":                                                     # taps reversed
            w = w.flip(-1)
        if mut == "g":                                                     # no left padding: the first tap reads frame 0 instead of zero
            x = F.conv1d(torch.cat([x[..., :1], x, torch.zeros_like(x[..., :1])], dim=-1), w, sd[key + ".bias"], stride=2)
        else:
            x = F.conv1d(x, w, sd[key + ".bias"], stride=2, padding=1)
        x = F.leaky_relu(x, slope)
    return F.linear(x.permute(0, 2, 1), sd["out_net.weight"], sd["out_net.bias"])


def gru_last(sd, x, lens, h0, mut=None, gates=None):
    B, T, _ = x.shape
    lens = torch.as_tensor(lens)
    outs = []
    for d, sfx in enumerate(("", "_reverse")):
        wi, wh = sd[f"gru.weight_ih_l0{sfx}"], sd[f"gru.weight_hh_l0{sfx}"]
        bi, bh = sd[f"gru.bias_ih_l0{sfx}"], sd[f"gru.bias_hh_l0{sfx}"]
        H = wh.shape[1]
        h = h0[0 if mut == "d" else d].expand(B, H).clone()                # (d): direction 1 starts from hidden[0]
        gi_all = F.linear(x, wi, bi)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            gi, gh = gi_all[:, t], F.linear(h, wh, bh)
            r = torch.sigmoid(gi[:, :H] + gh[:, :H])
            z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
            if mut == "b":                                                 # r and z swapped
                r, z = z, r
            if mut == "a":                                                 # b_hh of the n gate outside r * (...)
                n = torch.tanh(gi[:, 2 * H:] + r * (gh[:, 2 * H:] - bh[2 * H:]) + bh[2 * H:])
            else:
                n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
            hn = (1 - z) * n + z * h
            valid = (t < lens).unsqueeze(1)
            if gates is not None:
                gates.append(torch.cat([r[valid[:, 0]].flatten(), z[valid[:, 0]].flatten()]))
            if mut == "c" and d == 1:                                      # backward from T - 1: the state advances on padded steps
                h = hn
            else:
                h = torch.where(valid, hn, h)
        outs.append(h)
    return torch.cat(outs, dim=-1)


def head(sd, x, mut=None):
    x = F.linear(x, sd["output_net.0.weight"], sd["output_net.0.bias"])
    g, b = sd["output_net.1.weight"], sd["output_net.1.bias"]
    if mut == "h":                                                         # gamma / beta one channel off
        g, b = torch.roll(g, 1), torch.roll(b, 1)
    x = F.leaky_relu(F.layer_norm(x, (x.shape[-1],), g, b, 1e-5), 0.01 if mut == "e" else 0.2)
    return F.linear(x, sd["output_net.3.weight"], sd["output_net.3.bias"])


def motion(sd, mov, lens, mut=None, gates=None):
    emb = F.linear(mov, sd["input_emb.weight"], sd["input_emb.bias"])
    return head(sd, gru_last(sd, emb, lens, sd["hidden"][:, 0], mut, gates), mut)


def text(sd, w, pos, lens, mut=None, gates=None):
    emb = F.linear(w + F.linear(pos, sd["pos_emb.weight"], sd["pos_emb.bias"]), sd["input_emb.weight"], sd["input_emb.bias"])
    return head(sd, gru_last(sd, emb, lens, sd["hidden"][:, 0], mut, gates), mut)


def d64(sd):
    return {k: v.double() for k, v in sd.items()}


def shares(gates):
    g = torch.cat(gates)
    return ((g < 0.01) | (g > 0.99)).double().mean().item(), ((g >= 0.1) & (g <= 0.9)).double().mean().item()


def default_run(net, regime, gain=None):
    """(share saturated, share open, e32, max |embedding|, result) of a GRU network on its default case."""
    kw = {} if gain is None else {"motion_gain": float(gain), "text_gain": float(gain)}
    _, mo, tx = ev.evaluator_weights(263, regime, **kw)
    gates = []
    with torch.no_grad():
        if net == "motion":
            c, sd = ev.DEFAULT_MOTION, mo
            mov = ev.movements(c, regime)
            got = motion(d64(sd), mov.double(), c.lens, gates=gates)
            (want,), (e32,) = oracle_pair(ev.motion_fn(mov, c.lens), sd)
        else:
            c, sd = ev.DEFAULT_TEXT, tx
            w, pos = ev.words(c)
            got = text(d64(sd), w.double(), pos.double(), c.lens, gates=gates)
            (want,), (e32,) = oracle_pair(ev.text_fn(w, pos, c.lens), sd)
    assert torch.equal(got, want), "the restatement is the oracle"
    sat, mid = shares(gates)
    return sat, mid, e32, want.abs().max().item(), want


# ---------------------------------------------------------------- gate regime
@pytest.mark.parametrize("net", ["motion", "text"])
def test_gate_regime_of_both_weight_sets(net):
    sat, mid, e32, top, want = default_run(net, "synthetic")
    print(f"\n[evaluator cases] {net} synthetic: saturated {sat:.3f}  open {mid:.3f}  e32 {e32:.2e}  max|emb| {top:.2f}")
    assert torch.isfinite(want).all() and sat < 0.01 and e32 < E32_CAP * max(1.0, top)
    sat, mid, e32, top, want = default_run(net, "trained_like")
    print(f"[evaluator cases] {net} trained_like (gain {ev.MOTION_GAIN if net == 'motion' else ev.TEXT_GAIN}): saturated {sat:.3f}  "
          f"open {mid:.3f}  e32 {e32:.2e}  max|emb| {top:.2f}")
    assert torch.isfinite(want).all()
    assert sat >= SATURATED_SHARE and mid >= OPEN_SHARE, (net, sat, mid)
    assert e32 < E32_CAP * max(1.0, top), (net, e32, top)


@pytest.mark.parametrize("net", ["motion", "text"])
def test_the_gain_is_the_smallest_that_meets_both_shares(net):
    chosen = ev.MOTION_GAIN if net == "motion" else ev.TEXT_GAIN
    assert chosen in ev.GAINS
    for gain in ev.GAINS:
        if gain >= chosen:
            break
        sat, mid, e32, top, _ = default_run(net, "trained_like", gain)
        print(f"\n[evaluator cases] {net} gain {gain}: saturated {sat:.3f}  open {mid:.3f}  e32 {e32:.2e}  max|emb| {top:.2f}")
        assert not (sat >= SATURATED_SHARE and mid >= OPEN_SHARE), (net, gain, sat, mid)


# ---------------------------------------------------------------- e32 of every case
def _e32_ok(tag, fn, *sds):
    want, e32 = oracle_pair(fn, *sds)
    for w, e in zip(want, e32):
        top = w.abs().max().item()
        assert torch.isfinite(w).all() and e < E32_CAP * max(1.0, top), (tag, e, top)
    return max(e / max(1.0, w.abs().max().item()) for w, e in zip(want, e32))


@pytest.mark.parametrize("regime", ev.REGIMES)
@pytest.mark.parametrize("nfeats", ev.NFEATS)
@pytest.mark.parametrize("group", ["shapes", "large"])
def test_e32_of_the_movement_cases(group, nfeats, regime):
    mv = ev.evaluator_weights(nfeats, regime)[0]
    worst = max(_e32_ok((c.name, nfeats, regime), ev.movement_fn(ev.features(c)), mv)
                for c in (ev.movement_cases(nfeats) if group == "shapes" else ev.movement_big_cases(nfeats)))
    print(f"\n[evaluator cases] movement {group} C={nfeats} {regime}: largest e32 / scale {worst:.2e}")


@pytest.mark.parametrize("regime", ev.REGIMES)
@pytest.mark.parametrize("group", ["shapes", "large", "chain263", "chain251"])
def test_e32_of_the_motion_cases(group, regime):
    if group.startswith("chain"):
        c = ev.motion_big_case(int(group[5:]))
        mv, mo, _ = ev.evaluator_weights(c.nfeats, regime)
        worst = _e32_ok((c.name, "chain", regime), ev.chain_fn(ev.features(c, 4 * c.F), c.lens), mv, mo)
    else:
        mo = ev.evaluator_weights(263, regime)[1]
        worst = max(_e32_ok((c.name, regime), ev.motion_fn(ev.movements(c, regime), c.lens), mo)
                    for c in (ev.motion_cases() if group == "shapes" else [ev.motion_big_case()]))
    print(f"\n[evaluator cases] motion {group} {regime}: largest e32 / scale {worst:.2e}")


@pytest.mark.parametrize("regime", ev.REGIMES)
@pytest.mark.parametrize("group", ["shapes", "large"])
def test_e32_of_the_text_cases(group, regime):
    tx = ev.evaluator_weights(263, regime)[2]
    worst = max(_e32_ok((c.name, regime), ev.text_fn(*ev.words(c), c.lens), tx)
                for c in (ev.text_cases() if group == "shapes" else [ev.text_big_case()]))
    print(f"\n[evaluator cases] text {group} {regime}: largest e32 / scale {worst:.2e}")


# ---------------------------------------------------------------- the cases see the mistakes
MOVEMENT_SEES = ["F9-B3", "F75-B3"]
GRU_SEES = ["T18-B5-unsorted", "T49-B6-decreasing"]
TEXT_SEES = ["T12-B5-unsorted", "T20-B5-decreasing"]


def _moved(mut):
    """[(case tag, distance moved / bound)] of mutation `mut` over the listed cases, both weight sets."""
    out = []
    with torch.no_grad():
        for regime in ev.REGIMES:
            mv, mo, tx = ev.evaluator_weights(263, regime)
            if mut in "efg":
                for name in MOVEMENT_SEES:
                    c = ev.by_name(ev.movement_cases(263), name)
                    x = ev.features(c)
                    (want,), (e32,) = oracle_pair(ev.movement_fn(x), mv)
                    assert torch.equal(movement(d64(mv), x.double()), want)
                    out.append((f"movement {name} {regime}", (movement(d64(mv), x.double(), mut) - want).abs().max().item()
                                / bound(e32, want, "fp32")))
            if mut in "abcdeh":
                for name in GRU_SEES:
                    c = ev.by_name(ev.motion_cases(), name)
                    mov = ev.movements(c, regime)
                    (want,), (e32,) = oracle_pair(ev.motion_fn(mov, c.lens), mo)
                    assert torch.equal(motion(d64(mo), mov.double(), c.lens), want)
                    out.append((f"motion {name} {regime}", (motion(d64(mo), mov.double(), c.lens, mut) - want).abs().max().item()
                                / bound(e32, want, "fp32")))
                for name in TEXT_SEES:
                    c = ev.by_name(ev.text_cases(), name)
                    w, pos = ev.words(c)
                    (want,), (e32,) = oracle_pair(ev.text_fn(w, pos, c.lens), tx)
                    assert torch.equal(text(d64(tx), w.double(), pos.double(), c.lens), want)
                    out.append((f"text {name} {regime}", (text(d64(tx), w.double(), pos.double(), c.lens, mut) - want).abs().max().item()
                                / bound(e32, want, "fp32")))
    return out


@pytest.mark.parametrize("mut,what", [
    ("a", "b_hh of the n gate outside r * (...)"), ("b", "r and z swapped"), ("c", "backward direction from T - 1"),
    ("d", "direction 1 starts from hidden[0]"), ("e", "LeakyReLU slope 0.01"), ("f", "conv taps reversed"),
    ("g", "left padding dropped"), ("h", "LayerNorm gamma / beta one channel off")])
def test_the_cases_see_the_mistake(mut, what):
    moved = _moved(mut)
    print(f"\n[evaluator cases] ({mut}) {what}: " + "; ".join(f"{tag} {r:.0f} x bound" for tag, r in moved))
    assert moved and max(r for _, r in moved) > FACTOR, (mut, moved)
    # every listed case sees it, not only the best one
    assert min(r for _, r in moved) > FACTOR, (mut, moved)
