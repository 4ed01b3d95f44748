"""The multimodality metric and the test protocol on the CPU: `MMMetrics` against values recorded from the reference's
`calculate_multimodality_np` (tests/golden/make_golden_mm.py), the `test.py` statistics restated, `evaluate()` on a stub model, the
launch cutting of `LADIFF.mm_eval`, and the C-ABI declaration of `ladiff_gather_rows`."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ladiff_amd import LADIFF, MMMetrics, TM2TMetrics, _lib, evaluate, get_metric_statistics
from ladiff_amd import evaluation
from conftest import ROOT, load_golden


def _fed(g, tag, chunks=1, **kw):
    m = MMMetrics(mm_num_times=int(g[f"{tag}_times"]), **kw)
    act = g[f"{tag}_act"]
    for part in torch.chunk(act, chunks, dim=0):
        m.update(part, [60] * part.shape[0])
    return m


@pytest.mark.parametrize("tag,shape", [("main", (12, 30, 512)), ("edge", (1, 11, 512))])
def test_mm_metrics_reproduce_the_reference(tag, shape):
    """Fed the reference's two draws: its float64 result to 1e-12 relative (fp64 on both sides, the same sums up to their order) and its
    float32 result to 1e-5 relative (float32 rounding of a 512-term norm and a 120-term mean, with margin)."""
    g = load_golden("mm_metrics")
    assert tuple(g[f"{tag}_act"].shape) == shape and g[f"{tag}_act"].dtype == torch.float32
    m = _fed(g, tag)
    assert m.name == "MultiModality scores" and m.metrics == ["MultiModality"]
    out = m.compute(False, first=g[f"{tag}_first"].numpy(), second=g[f"{tag}_second"].numpy())
    assert list(out) == ["MultiModality"]
    v64, v32 = float(g[f"{tag}_value64"]), float(g[f"{tag}_value32"])
    rel64, rel32 = abs(out["MultiModality"] - v64) / v64, abs(out["MultiModality"] - v32) / v32
    print(f"{tag}: MultiModality {out['MultiModality']!r}; vs reference float64 {rel64:.2e}, vs reference float32 {rel32:.2e}")
    assert rel64 <= 1e-12
    assert rel32 <= 1e-5
    assert m.count_seq == shape[0] and m.count == 60 * shape[0]


def test_mm_metrics_update_in_one_batch_or_twelve():
    g = load_golden("mm_metrics")
    first, second = g["main_first"].numpy(), g["main_second"].numpy()
    one = _fed(g, "main").compute(False, first=first, second=second)
    twelve = _fed(g, "main", chunks=12)
    assert len(twelve._mm) == 12 and twelve.count_seq == 12
    assert twelve.compute(False, first=first, second=second) == one


def test_mm_metrics_asserts_sanity_and_seeds():
    g = load_golden("mm_metrics")
    with pytest.raises(AssertionError):                       # R = 11 repeats need mm_num_times < 11
        MMM = MMMetrics(mm_num_times=11)
        MMM.update(g["edge_act"], [60])
        MMM.compute(False)
    with pytest.raises(AssertionError):                       # R == mm_num_times
        MMM = MMMetrics(mm_num_times=30)
        MMM.update(g["main_act"], [60] * 12)
        MMM.compute(False)
    with pytest.raises(AssertionError):                       # 3-D input only
        MMM = MMMetrics(mm_num_times=10)
        MMM.update(g["main_act"].reshape(360, 512), [60] * 360)
        MMM.compute(False)
    assert _fed(g, "main").compute(sanity_flag=True) == {"MultiModality": 0.0}
    a, b, c = (_fed(g, "main", seed=s).compute(False)["MultiModality"] for s in (3, 3, 4))
    assert a == b and a != c and a > 0
    m = MMMetrics(mm_num_times=10, dist_sync_on_step=True)    # the reference's constructor kwargs
    assert m.mm_num_times == 10


def test_get_metric_statistics_restated():
    """`test.py:32-36`: mean and 1.96 * population std / sqrt(n), by hand for [1, 2, 3, 4]: mean 2.5, std sqrt(1.25)."""
    mean, conf = get_metric_statistics(np.array([1.0, 2.0, 3.0, 4.0]), 4)
    assert mean == 2.5 and abs(conf - 1.96 * np.sqrt(1.25) / 2.0) < 1e-15
    mean, conf = get_metric_statistics(np.array([[1.0, 10.0], [3.0, 10.0]]), 2)        # axis 0: per column
    assert mean.tolist() == [2.0, 10.0] and np.allclose(conf, [1.96 * 1.0 / np.sqrt(2.0), 0.0], rtol=0, atol=1e-15)
    mean, conf = get_metric_statistics(np.array([7.0]), 1)
    assert mean == 7.0 and conf == 0.0


class _StubModel:
    """Fixed embeddings per replication; records the order of the calls."""

    def __init__(self, n_seq=40, n_mm=3, R=30):
        self.calls, self.rep, self.R = [], 0, R
        rs = np.random.RandomState(1)
        self.text = torch.from_numpy(rs.standard_normal((n_seq, 512)))
        self.noise = torch.from_numpy(rs.standard_normal((2, n_seq, 512)))
        self.mm = torch.from_numpy(rs.standard_normal((2, n_mm, R, 512)))

    def t2m_eval(self, batch):
        self.calls.append(("t2m", tuple(batch["id"])))
        if batch["id"][0] == 0:
            self.rep = sum(1 for c in self.calls if c == ("t2m", tuple(batch["id"]))) - 1
        ids = torch.tensor(batch["id"])
        return {"lat_t": self.text[ids], "lat_rm": (self.text + self.noise[self.rep])[ids], "lat_m": self.text[ids] * 1.01}

    def mm_eval(self, batch):
        self.calls.append(("mm", tuple(batch["id"])))
        return {"lat_rm": self.mm[self.rep][torch.tensor(batch["id"])], "lengths": [l for l in batch["length"] for _ in range(self.R)]}


def test_evaluate_runs_the_passes_in_the_reference_s_order_and_aggregates():
    model = _StubModel()
    tm_batches = [{"id": list(range(i, i + 8)), "length": [60] * 8} for i in range(0, 40, 8)]
    mm_batches = [{"id": [i], "length": [60]} for i in range(3)]
    mk = lambda: (TM2TMetrics(top_k=3, R_size=8, diversity_times=20, seed=5), MMMetrics(mm_num_times=10, seed=6))
    stats, per = evaluate(model, tm_batches, mm_batches, replication_times=2, metrics=mk())
    one_rep = [("t2m", tuple(b["id"])) for b in tm_batches] + [("mm", tuple(b["id"])) for b in mm_batches]
    assert model.calls == one_rep + one_rep                     # TM2T pass, then MM pass, per replication (test.py:138-147)
    assert set(per) == set(TM2TMetrics(top_k=3).metrics) | {"MultiModality"}
    assert all(len(v) == 2 for v in per.values())
    # the same numbers from the metric classes driven by hand (one generator per class, continuing over the replications)
    tm, mm = mk()
    for rep in range(2):
        tm.reset(); mm.reset()
        tm.update(model.text, model.text + model.noise[rep], model.text * 1.01, [60] * 40)
        mm.update(model.mm[rep], [60] * 90)
        want = {**tm.compute(), **mm.compute()}
        for k, v in want.items():
            assert per[k][rep] == pytest.approx(v, rel=1e-12, abs=1e-12), k
    for k, v in per.items():
        mean, conf = stats[k]
        assert mean == pytest.approx(np.mean(v)) and conf == pytest.approx(1.96 * np.std(v) / np.sqrt(2))
    assert per["MultiModality"][0] != per["MultiModality"][1] and stats["MultiModality"][1] > 0
    # no MM batches: the TM2T columns alone
    stats, per = evaluate(_StubModel(), tm_batches, None, replication_times=1, metrics=mk())
    assert "MultiModality" not in per and stats["FID"][1] == 0.0
    with pytest.raises(ValueError):
        evaluate(model, tm_batches, mm_batches, replication_times=0)
    assert evaluation.evaluate is evaluate


@pytest.mark.parametrize("cap", [320, 64])
@pytest.mark.parametrize("B", [1, 7, 8, 9, 100])
def test_mm_launch_cutting(B, cap):
    """Whole prompts per launch, at most `max_prompts_per_launch` motions, exact cover in order."""
    R = 30
    owner = SimpleNamespace(max_prompts_per_launch=cap)
    spans = LADIFF._mm_launches(owner, B, R)
    assert spans[0][0] == 0 and spans[-1][1] == B
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))                  # contiguous, no overlap: the cover is exact
    assert all(hi > lo and (hi - lo) * R <= cap for lo, hi in spans)            # whole prompts, <= cap motions
    assert len(spans) == -(-B // (cap // R))                                    # no more launches than needed
    assert max(hi - lo for lo, hi in spans) - min(hi - lo for lo, hi in spans) <= 1
    for ppl in (1, 3):
        cut = LADIFF._mm_launches(owner, B, R, prompts_per_launch=ppl)
        assert cut[0][0] == 0 and cut[-1][1] == B and all(a[1] == b[0] for a, b in zip(cut, cut[1:]))
        assert all(0 < hi - lo <= min(ppl, cap // R) for lo, hi in cut)
    if cap == 320:
        assert LADIFF._mm_launches(owner, B, R, prompts_per_launch=1000) == spans       # never above the cap


def test_mm_launch_cutting_defaults_and_odd_cases():
    from ladiff_amd import DDIMScheduler, LADiffDenoiser, LADiffVae
    from ladiff_amd.schema import ABL, DEN_KW, VAE_KW
    sch = DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                        clip_sample=False, set_alpha_to_one=False, steps_offset=1)
    model = LADIFF(denoiser=LADiffDenoiser(ABL, **DEN_KW), vae=LADiffVae(ABL, **VAE_KW), scheduler=sch)
    assert model.max_prompts_per_launch == 320 and model.mm_num_repeats == 30
    assert model._mm_launches(100, 30) == [(10 * i, 10 * i + 10) for i in range(10)]
    cfg_model = LADIFF({"TEST": {"MM_NUM_REPEATS": 7}}, denoiser=model.denoiser, vae=model.vae, scheduler=sch)
    assert cfg_model.mm_num_repeats == 7
    assert LADIFF({"TEST": {"MM_NUM_REPEATS": 7}}, denoiser=model.denoiser, vae=model.vae, scheduler=sch, mm_num_repeats=3).mm_num_repeats == 3
    # more repeats than the cap: one prompt per launch (the loop cuts its samples); no cap: one launch
    assert LADIFF._mm_launches(SimpleNamespace(max_prompts_per_launch=16), 3, 30) == [(0, 1), (1, 2), (2, 3)]
    assert LADIFF._mm_launches(SimpleNamespace(max_prompts_per_launch=None), 50, 30) == [(0, 50)]


def test_gather_rows_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "ladiff_hip.h")).read()
    decl = re.search(r"LADIFF_API int ladiff_gather_rows\(([^)]*)\)", src)
    assert decl is not None
    assert [a.strip() for a in decl.group(1).split(",")] == ["const float* src", "const int32_t* index", "int n_rows", "int row_floats",
                                                             "float* dst", "ladiff_stream_t stream"]
    assert "ladiff_gather_rows" in _lib.EXPORTS
    from ladiff_amd import build
    build.build()
    lib = _lib.lib()
    assert hasattr(lib, "ladiff_gather_rows") and lib.ladiff_version() == 6
    # argument errors are answered on the host, before anything is launched
    assert lib.ladiff_gather_rows(None, None, 4, 768, None, None) == -1
    assert lib.ladiff_gather_rows(None, None, -1, 768, None, None) == -1
    assert lib.ladiff_gather_rows(None, None, 0, 768, None, None) == 0
    assert lib.ladiff_gather_rows(16, 16, 4, 770, 16, None) == -2            # rows that are not whole 16-byte chunks
    assert lib.ladiff_gather_rows(20, 16, 4, 768, 16, None) == -2            # src not 16-byte aligned
    with pytest.raises(_lib.LadiffHipError):
        _lib.gather_rows(torch.zeros(4, 768), [0, 1])                        # CPU tensor: no fallback
