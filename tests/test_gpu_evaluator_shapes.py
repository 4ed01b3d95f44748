"""The T2M evaluator encoders (csrc/evaluator.hip: movement conv encoder, motion bi-GRU, text bi-GRU) against the fp64 oracle over the
shapes, GEMM routes and gate regimes that decide which code runs.  Every headline metric is computed from these embeddings.

* GEMM routes by row count (csrc/gemm.hip `launch_gemm`): fp32 products with M >= 4096 and N % 128 == 0 go to the LDS-DMA kernel of
  gemm_big.hip, M >= 4096 otherwise to the 128 x 128 staged tile, smaller ones to the 64 x 64 / 32 x 32 tiles.  `mm_eval` sends all repeats
  of the prompts of one length through the encoders together, so the conv (K = 1056 / 2048, LeakyReLU), input-projection and gi products
  (N = 1024 / 3072 / 512 / 1536) take the large route there.  B = 42 / 84 at F = 196 give 4,116 rows to conv0 / to conv3 and out_net,
  B = 41 / 83 stay just below; B = 84 at T = 49 and B = 205 at L = 20 do the same for the GRU networks (M = 4,116 / 4,100).
* the small kernels (im2col, gru_gate / init / cat, ln_lrelu) are reached through the modules only: F = 4 .. 9 (T2 = 1 or 2, odd T1),
  B = 1, B = 5 / 6 at the ln_lrelu row guard, T = 1 and L = 1, all lengths 1, all lengths T, a different backward start for every sample.
* both weight sets of tests/evaluator_cases.py: synthetic (gates near 0.5: indexing shows at full size) and trained-like (a fifth to a third
  of the gates saturated, spread LayerNorm, biases of size 0.3).

Every comparison: `trained_like.oracle_pair` for (want, e32), then err <= `trained_like.bound(e32, want, "fp32")` = 8 e32 + 1e-6 scale; the
oracle of a case is computed once.  Every call is made twice and must give the same bits.  `pytest -s` prints err, e32, err / e32 and the
bound of every result; DESIGN.md section 6 records what an MI355X showed (largest err / e32 of a module 4.31, of the large-M cases 3.36)."""
import pytest
import torch

from ladiff_amd import MotionEncoderBiGRUCo, MovementConvEncoder, TextEncoderBiGRUCo, _lib
from trained_like import bound
from test_gpu_trained_like import check, oracle

import evaluator_cases as ev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_NETS = {}


def nets(nfeats, regime):
    key = (nfeats, regime)
    if key not in _NETS:
        mv, mo, tx = ev.evaluator_weights(nfeats, regime)
        move = MovementConvEncoder(nfeats - 4, 512, 512); move.load_state_dict(mv, strict=True)
        motion = MotionEncoderBiGRUCo(512, 1024, 512); motion.load_state_dict(mo, strict=True)
        text = TextEncoderBiGRUCo(300, 15, 512, 512); text.load_state_dict(tx, strict=True)
        _NETS[key] = (move.to(DEV), motion.to(DEV), text.to(DEV))
    return _NETS[key]


def twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    assert torch.equal(a, b), "the same call twice gives the same bits"
    return a


# ---------------------------------------------------------------- runners: GPU result of a case, checked against its oracle
def run_movement(c, regime, group="shapes"):
    x = ev.features(c)
    (want,), (e32,) = oracle(("eval-move", regime, c), ev.movement_fn(x), ev.evaluator_weights(c.nfeats, regime)[0])
    move = nets(c.nfeats, regime)[0]
    xd = x.to(DEV)
    view = xd[..., :-4]                                            # the strided view `t2m_eval` passes
    assert not view.is_contiguous()
    got = twice(lambda: move(view))
    assert torch.equal(got, move(view.contiguous())), (c.name, "strided view and contiguous tensor differ")
    check(f"evaluator {group} | movement {c.name} C={c.nfeats} {regime}", "fp32", got, want, e32)
    return got


def run_motion(c, regime, group="shapes"):
    mov = ev.movements(c, regime)
    (want,), (e32,) = oracle(("eval-motion", regime, c), ev.motion_fn(mov, c.lens), ev.evaluator_weights(c.nfeats, regime)[1])
    motion = nets(c.nfeats, regime)[1]
    md = mov.to(DEV)
    got = twice(lambda: motion(md, torch.tensor(c.lens)))
    check(f"evaluator {group} | motion {c.name} {regime}", "fp32", got, want, e32)
    return got, want, e32


def run_text(c, regime, group="shapes"):
    w, pos = ev.words(c)
    (want,), (e32,) = oracle(("eval-text", regime, c), ev.text_fn(w, pos, c.lens), ev.evaluator_weights(c.nfeats, regime)[2])
    text = nets(c.nfeats, regime)[2]
    wd, pd = w.to(DEV), pos.to(DEV)
    got = twice(lambda: text(wd, pd, torch.tensor(c.lens)))
    check(f"evaluator {group} | text {c.name} {regime}", "fp32", got, want, e32)
    return got, want, e32


# ---------------------------------------------------------------- movement encoder
@pytest.mark.parametrize("regime", ev.REGIMES)
@pytest.mark.parametrize("nfeats", ev.NFEATS)
@pytest.mark.parametrize("name", [c.name for c in ev.movement_cases(263)])
def test_movement_shapes(name, nfeats, regime):
    """F = 4 .. 9: T1 = 2 .. 4 (odd at F = 6, 7), T2 = 1 or 2; F = 75: no multiple of 4; B = 1 and 3."""
    c = ev.by_name(ev.movement_cases(nfeats), name)
    got = run_movement(c, regime)
    assert got.shape == (c.B, c.F // 2 // 2, 512)


def test_movement_refuses_fewer_than_4_frames():
    move = nets(263, "synthetic")[0]
    with pytest.raises(_lib.LadiffHipError):
        move(torch.zeros(2, 3, 263, device=DEV)[..., :-4])


@pytest.mark.parametrize("regime", ev.REGIMES)
@pytest.mark.parametrize("nfeats", ev.NFEATS)
@pytest.mark.parametrize("B", ev.MOVE_BIG_B)
def test_movement_large_route(B, nfeats, regime):
    """F = 196.  B = 42: conv0 (K = 1056 at nfeats 263: 33 K stages; 992 at 251; LeakyReLU) has 4,116 rows = 32 tiles of 128 + 20 rows.
    B = 84: conv3 (K = 2048, LeakyReLU) and out_net have 4,116.  B = 41 / 83: the same products just below the route change."""
    run_movement(ev.by_name(ev.movement_big_cases(nfeats), f"F196-B{B}"), regime, "large-M")


# ---------------------------------------------------------------- motion encoder
@pytest.mark.parametrize("regime", ev.REGIMES)
@pytest.mark.parametrize("name", [c.name for c in ev.motion_cases()])
def test_motion_shapes(name, regime):
    run_motion(ev.by_name(ev.motion_cases(), name), regime)


@pytest.mark.parametrize("regime", ev.REGIMES)
def test_motion_large_route(regime):
    """B = 84, T = 49, lengths cycling over 49 / 30 / 12 / 1: input_emb (N = 1024, K = 512) and both gi products (N = 3072, K = 1024) have
    4,116 rows; the per-step products have 84."""
    run_motion(ev.motion_big_case(), regime, "large-M")


# ---------------------------------------------------------------- text encoder
@pytest.mark.parametrize("regime", ev.REGIMES)
@pytest.mark.parametrize("name", [c.name for c in ev.text_cases()])
def test_text_shapes(name, regime):
    run_text(ev.by_name(ev.text_cases(), name), regime)


@pytest.mark.parametrize("regime", ev.REGIMES)
def test_text_large_route(regime):
    """B = 205, L = 20: M = 4,100.  input_emb (N = 512, K = 320) and gi (N = 1536, K = 512) on the large-M kernel, the POS product (N = 300,
    K = 32, ldy = 320, residual) on the 128 x 128 staged tile."""
    run_text(ev.text_big_case(), regime, "large-M")


# ---------------------------------------------------------------- padding never reaches an embedding
@pytest.mark.parametrize("regime", ev.REGIMES)
def test_rows_behind_a_length_never_reach_the_embedding(regime):
    """The gi rows of padded steps are computed and must never be read: zeros, 1e30 and NaN behind each length give the same bits."""
    _, motion, text = nets(263, regime)
    c = ev.by_name(ev.motion_cases(), "T18-B5-unsorted")
    mov, lens = ev.movements(c, regime), torch.tensor(c.lens)
    got = [motion(ev.pad_fill(mov, c.lens, v).to(DEV), lens) for v in (0.0, 1e30, float("nan"))]
    assert torch.isfinite(got[0]).all() and torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    assert torch.equal(got[0], motion(mov.to(DEV), lens))
    c = ev.by_name(ev.text_cases(), "T12-B5-unsorted")
    (w, pos), lens = ev.words(c), torch.tensor(c.lens)
    got = [text(ev.pad_fill(w, c.lens, v).to(DEV), ev.pad_fill(pos, c.lens, v).to(DEV), lens) for v in (0.0, 1e30, float("nan"))]
    assert torch.isfinite(got[0]).all() and torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    assert torch.equal(got[0], text(w.to(DEV), pos.to(DEV), lens))


# ---------------------------------------------------------------- order and batch independence
@pytest.mark.parametrize("regime", ev.REGIMES)
def test_permuting_the_samples_permutes_the_embeddings(regime):
    """Same B, same routes: bit-exact."""
    move, motion, text = nets(263, regime)
    perm = torch.tensor([3, 0, 4, 2, 1])
    c = ev.by_name(ev.motion_cases(), "T18-B5-unsorted")
    mov, lens = ev.movements(c, regime).to(DEV), torch.tensor(c.lens)
    assert torch.equal(motion(mov, lens)[perm], motion(mov[perm], lens[perm]))
    c = ev.by_name(ev.text_cases(), "T12-B5-unsorted")
    (w, pos), lens = ev.words(c), torch.tensor(c.lens)
    assert torch.equal(text(w.to(DEV), pos.to(DEV), lens)[perm], text(w[perm].to(DEV), pos[perm].to(DEV), lens[perm]))
    c = ev.by_name(ev.movement_cases(263), "F75-B3")
    x, p3 = ev.features(c).to(DEV)[..., :-4], torch.tensor([2, 0, 1])
    assert torch.equal(move(x)[p3], move(x[p3]))


@pytest.mark.parametrize("regime", ev.REGIMES)
def test_a_sample_alone_equals_its_row_of_the_large_batch(regime):
    """B = 84 runs on the large-M route, B = 1 on the small tiles: other kernels, so the rows are asked to agree within the bound, not in
    bits (an MI355X gave the same bits all the same).  One sample of every length of the motion batch, and its last sample; the first and
    the last sample of the movement batch."""
    move, motion, _ = nets(263, regime)
    c = ev.motion_big_case()
    batch, want, e32 = run_motion(c, regime, "large-M")
    b = bound(e32, want, "fp32")
    mov = ev.movements(c, regime).to(DEV)
    for i in (0, 1, 2, 3, 83):
        alone = motion(mov[i:i + 1], torch.tensor(c.lens[i:i + 1]))
        err = (alone[0].double() - batch[i].double()).abs().max().item()
        print(f"[evaluator alone] motion sample {i} (length {c.lens[i]}) {regime}: |alone - batch row| {err:.3e}  bound {b:.3e}")
        assert err <= b, (i, err, b)
    c = ev.by_name(ev.movement_big_cases(263), "F196-B84")
    x = ev.features(c)
    (want,), (e32,) = oracle(("eval-move", regime, c), ev.movement_fn(x), ev.evaluator_weights(263, regime)[0])
    b = bound(e32, want, "fp32")
    xd = x.to(DEV)[..., :-4]
    batch = move(xd)
    for i in (0, 83):
        err = (move(xd[i:i + 1])[0].double() - batch[i].double()).abs().max().item()
        print(f"[evaluator alone] movement sample {i} {regime}: |alone - batch row| {err:.3e}  bound {b:.3e}")
        assert err <= b, (i, err, b)


# ---------------------------------------------------------------- the chain mm_eval runs
@pytest.mark.parametrize("regime", ev.REGIMES)
@pytest.mark.parametrize("nfeats", ev.NFEATS)
def test_movement_into_motion_at_the_large_size(nfeats, regime):
    """feats -> movement encoder -> motion encoder on the GPU's own movements, B = 84, F = 196, lengths 196 / 120 / 48 / 4 frames cycling,
    against the oracle's chain."""
    c = ev.motion_big_case(nfeats)
    x = ev.features(c, 4 * c.F)
    mv, mo, _ = ev.evaluator_weights(nfeats, regime)
    (want_mov, want_emb), (e_mov, e_emb) = oracle(("eval-chain", regime, c), ev.chain_fn(x, c.lens), mv, mo)
    move, motion, _ = nets(nfeats, regime)
    xd = x.to(DEV)
    mov = twice(lambda: move(xd[..., :-4]))
    emb = twice(lambda: motion(mov, torch.tensor(c.lens)))
    check(f"evaluator chain | movements B=84 C={nfeats} {regime}", "fp32", mov, want_mov, e_mov)
    check(f"evaluator chain | motion embedding B=84 C={nfeats} {regime}", "fp32", emb, want_emb, e_emb)
