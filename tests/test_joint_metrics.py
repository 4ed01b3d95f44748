"""The joint-space metrics on the CPU: the numpy restatement (tests/joint_metrics_ref.py) against values recorded from the reference's
`ComputeMetrics` and `MRMetrics` (tests/golden/make_golden_joint_metrics.py), the `compute()` arithmetic of the two classes on
hand-made sums, `evaluate(..., joint_metrics=...)` on a stub model, and the C-ABI declarations of the two entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import joint_metrics_ref as ref
from ladiff_amd import ComputeMetrics, MMMetrics, MRMetrics, TemosMetric, TM2TMetrics, _lib, evaluate
from ladiff_amd.joint_metrics import PART_INDEX
from conftest import ROOT, load_golden

CASES = {"a": (5, 196, 22, [196, 65, 64, 2, 120], "humanml3d"), "b": (3, 70, 21, [70, 33, 3], "humanml3d"),
         "c": (2, 3, 22, [3, 2], "humanml3d"), "d": (5, 196, 22, [196, 65, 64, 2, 120], "mmm")}
APE_KEYS = ["APE_root", "APE_traj", "APE_mean_pose", "APE_mean_joints", "AVE_root", "AVE_traj", "AVE_mean_pose", "AVE_mean_joints"]
MR_KEYS = ["MPJPE", "PAMPJPE", "ACCEL"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_reproduces_the_reference_in_float64(case):
    """Two double-precision evaluations of the same formulas differ by rounding only: 1e-9 relative, per sequence and in total."""
    g = load_golden("joint_metrics")
    B, F, J, lengths, jointstype = CASES[case]
    rst, rf = g[f"{case}_rst"].numpy(), g[f"{case}_ref"].numpy()
    assert rst.shape == rf.shape == (B, F, J, 3) and rst.dtype == np.float32 and g[f"{case}_lengths"].tolist() == lengths
    assert str(g[f"{case}_jointstype"]) == jointstype
    assert tuple(g[f"{case}_parts"].tolist()) == ref.PARTS[jointstype] == PART_INDEX[jointstype]        # the golden pins the eight positions
    assert list(g["ape_keys"]) == APE_KEYS and list(g["mr_keys"]) == MR_KEYS
    ape, mr = ref.ape_ave_rows(rst, rf, lengths, jointstype), ref.mr_rows(rst, rf)
    want_ape, want_mr = g[f"{case}_ape_rows64"].numpy(), g[f"{case}_mr_rows64"].numpy()
    assert ape.shape == want_ape.shape == (B, 4 + 2 * (J - 1) + 2 * J) and mr.shape == want_mr.shape == (B, 3)
    rel = lambda got, want: float(np.max(np.abs(got - want) / np.abs(want)))
    total_ape = ref.ape_ave_compute(ape.sum(axis=0), sum(lengths), B, J)
    total_mr = ref.mr_compute(mr.sum(axis=0), sum(lengths), B)
    assert list(total_ape) == APE_KEYS and list(total_mr) == MR_KEYS
    figures = {"ape rows": rel(ape, want_ape), "mr rows": rel(mr, want_mr),
               "ape compute": rel(np.array(list(total_ape.values())), g[f"{case}_ape_compute64"].numpy()),
               "mr compute": rel(np.array(list(total_mr.values())), g[f"{case}_mr_compute64"].numpy())}
    print(case, figures)
    assert all(v <= 1e-9 for v in figures.values()), figures


def test_compute_arithmetic_on_hand_made_sums():
    """Divisors, key names and the popped arrays (compute.py:71-100, mr.py:52-71), through add_sums."""
    J = 22
    m = ComputeMetrics(njoints=J, jointstype="humanml3d")
    assert TemosMetric is ComputeMetrics and m.name == "APE and AVE"
    assert m.metrics == ["APE_root", "APE_traj", "APE_pose", "APE_joints", "AVE_root", "AVE_traj", "AVE_pose", "AVE_joints"]
    assert m.factor == 1000.0 * 0.75 / 480.0 and ComputeMetrics(njoints=21).factor == 1000.0
    assert ComputeMetrics(njoints=J, jointstype="humanml3d", force_in_meter=False).factor == 1.0
    W = 4 + 2 * (J - 1) + 2 * J
    sums = np.concatenate([[10.0, 20.0], np.arange(1, J), np.arange(1, J + 1) * 2.0, [3.0, 6.0], np.arange(1, J) * 3.0, np.arange(1, J + 1) * 4.0])
    assert sums.shape == (W,)
    m.add_sums({"count": 40, "count_seq": 2, "sums": sums})
    m.add_sums({"count": 10, "count_seq": 1, "sums": sums})                   # the reference's dist_reduce_fx="sum"
    out = m.compute(sanity_flag=False)
    assert list(out) == APE_KEYS
    want = {"APE_root": 20.0 / 50, "APE_traj": 40.0 / 50, "APE_mean_pose": 2 * 11.0 / 50, "APE_mean_joints": 2 * 23.0 / 50,
            "AVE_root": 6.0 / 3, "AVE_traj": 12.0 / 3, "AVE_mean_pose": 2 * 33.0 / 3, "AVE_mean_joints": 2 * 46.0 / 3}
    assert out == pytest.approx(want, rel=1e-15)
    st = m.sums()
    assert st["count"] == 50 and st["count_seq"] == 3 and np.array_equal(st["sums"], 2 * sums)
    other = ComputeMetrics(njoints=J, jointstype="humanml3d")
    other.add_sums(m)                                                          # an object merges like its sums()
    assert other.compute() == out
    m.reset()
    assert m.sums()["count"] == 0 and not m.sums()["sums"].any()
    with pytest.raises(ValueError):
        m.add_sums({"count": 1, "count_seq": 1, "sums": np.zeros(3)})

    r = MRMetrics(njoints=J, jointstype="humanml3d")
    assert r.name == "Motion Reconstructions" and r.metrics == MR_KEYS
    r.add_sums({"count": 100, "count_seq": 4, "sums": np.array([5.0, 2.5, 9.2])})
    assert r.compute(sanity_flag=False) == pytest.approx({"MPJPE": 50.0, "PAMPJPE": 25.0, "ACCEL": 100.0}, rel=1e-15)
    assert list(r.compute()) == MR_KEYS
    q = MRMetrics(njoints=J, jointstype="mmm", force_in_meter=False, dist_sync_on_step=True)
    q.add_sums(r)
    assert q.compute() == pytest.approx({"MPJPE": 0.05, "PAMPJPE": 0.025, "ACCEL": 0.1}, rel=1e-15)
    with pytest.raises(NotImplementedError):
        MRMetrics(njoints=J, align_root=False)
    for cls in (ComputeMetrics, MRMetrics):
        with pytest.raises(NotImplementedError):
            cls(njoints=J, jointstype="smplh")


def test_update_has_no_cpu_implementation():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for m in (ComputeMetrics(njoints=22, jointstype="humanml3d"), MRMetrics(njoints=22, jointstype="humanml3d")):
        with pytest.raises(_lib.LadiffHipError):
            m.update(torch.zeros(2, 8, 22, 3), torch.zeros(2, 8, 22, 3), [8, 8])
        with pytest.raises(_lib.LadiffHipError):
            m.update(torch.zeros(2, 8, 66), torch.zeros(2, 8, 66), [8, 8])                  # 3-D
        with pytest.raises(_lib.LadiffHipError):
            m.update(torch.zeros(2, 8, 22, 3), torch.zeros(2, 9, 22, 3), [8, 8])            # mismatched
        assert m.count == 0 and m.count_seq == 0


class _StubJointMetric:
    """Records what evaluate() hands it; `compute()` tells the replication and the number of sequences seen since the last reset."""

    def __init__(self, key):
        self.key, self.resets, self.seen, self.lengths = key, 0, 0, []

    def reset(self):
        self.resets += 1
        self.seen = 0

    def update(self, joints_rst, joints_ref, lengths):
        assert joints_rst.shape == joints_ref.shape and joints_rst.shape[0] == len(lengths)
        self.lengths.append(lengths)
        self.seen += len(lengths)

    def compute(self, sanity_flag=False):
        return {self.key: float(self.resets * 1000 + self.seen)}


class _StubModel:
    def __init__(self, n_seq=40):
        rs = np.random.RandomState(1)
        self.text = torch.from_numpy(rs.standard_normal((n_seq, 512)))
        self.noise = torch.from_numpy(rs.standard_normal((n_seq, 512)))

    def t2m_eval(self, batch):
        ids = torch.tensor(batch["id"])
        joints = torch.zeros(len(batch["id"]), 60, 22, 3)
        return {"lat_t": self.text[ids], "lat_rm": (self.text + self.noise)[ids], "lat_m": self.text[ids] * 1.01,
                "joints_rst": joints, "joints_ref": joints + 1}


def test_evaluate_feeds_resets_and_merges_joint_metrics():
    tm_batches = [{"id": list(range(i, i + 8)), "length": [60 - j for j in range(8)]} for i in range(0, 40, 8)]
    mk = lambda: (TM2TMetrics(top_k=3, R_size=8, diversity_times=20, seed=5), MMMetrics(mm_num_times=10, seed=6))
    a, b = _StubJointMetric("JM_A"), _StubJointMetric("JM_B")
    stats, per = evaluate(_StubModel(), tm_batches, None, replication_times=2, metrics=mk(), joint_metrics=iter([a, b]))
    assert set(per) == set(TM2TMetrics(top_k=3).metrics) | {"JM_A", "JM_B"}
    assert per["JM_A"] == per["JM_B"] == [1040.0, 2040.0]                       # reset per replication, all 40 sequences in each
    assert a.resets == 2 and len(a.lengths) == 10
    assert all(got is batch["length"] for got, batch in zip(a.lengths, tm_batches + tm_batches))       # the untouched batch["length"]
    assert stats["JM_A"] == (pytest.approx(1540.0), pytest.approx(1.96 * 500.0 / np.sqrt(2)))
    # joint_metrics=None: exactly the dict of a call without the argument
    plain = evaluate(_StubModel(), tm_batches, None, replication_times=2, metrics=mk())
    with_none = evaluate(_StubModel(), tm_batches, None, replication_times=2, metrics=mk(), joint_metrics=None)
    assert with_none == plain and set(plain[1]) == set(TM2TMetrics(top_k=3).metrics)
    assert {k: v for k, v in per.items() if not k.startswith("JM_")} == plain[1]


def test_joint_metric_entries_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "ladiff_hip.h")).read()
    flat = re.sub(r"\s+", " ", src)
    ape = re.search(r"LADIFF_API int ladiff_joint_ape_ave\(([^)]*)\)", flat)
    mr = re.search(r"LADIFF_API int ladiff_joint_mr\(([^)]*)\)", flat)
    assert ape is not None and mr is not None
    assert [a.strip() for a in ape.group(1).split(",")] == [
        "const float* joints_rst", "const float* joints_ref", "const int32_t* lengths", "const int32_t* h_lengths", "int B", "int F", "int J",
        "const int32_t* h_part_idx", "float factor", "float* seq_rows", "double* acc", "ladiff_stream_t stream"]
    assert [a.strip() for a in mr.group(1).split(",")] == [
        "const float* joints_rst", "const float* joints_ref", "const int32_t* h_lengths", "int B", "int F", "int J", "float* seq_rows",
        "double* acc", "ladiff_stream_t stream"]
    for needle in ("compute.py:102-196", "rifke.py:27-91", "mr.py:73-96", "utils.py:267-318"):                # each cites the reference
        assert needle in src, needle
    assert "ladiff_joint_ape_ave" in _lib.EXPORTS and "ladiff_joint_mr" in _lib.EXPORTS
    from ladiff_amd import build
    assert "joint_metrics.hip" in build.SOURCES
    build.build()
    lib = _lib.lib()
    assert hasattr(lib, "ladiff_joint_ape_ave") and hasattr(lib, "ladiff_joint_mr") and lib.ladiff_version() == 6
    # refusals are answered on the host, before anything is launched: the pointers here are never followed
    parts = (ctypes.c_int32 * 8)(*PART_INDEX["humanml3d"])
    pp = ctypes.cast(parts, ctypes.c_void_p)

    def lens(*v):
        return ctypes.cast((ctypes.c_int32 * len(v))(*v), ctypes.c_void_p)

    def ape_call(B=2, F=8, J=22, h=None, rst=16, acc=16, rows=16, parts=pp):
        return lib.ladiff_joint_ape_ave(rst, 16, 16, h if h is not None else lens(8, 8), B, F, J, parts, 1.0, rows, acc, None)

    def mr_call(B=2, F=8, J=22, h=None, rst=16, acc=16):
        return lib.ladiff_joint_mr(rst, 16, h if h is not None else lens(8, 8), B, F, J, 16, acc, None)

    for call in (ape_call, mr_call):
        assert call(B=0) == 0 and call(B=-1) == -1 and call(rst=None) == -1
        assert call(J=20) == -2 and call(J=23) == -2
        assert call(F=0) == -2 and call(F=225) == -2
        assert call(h=lens(8, 0)) == -2 and call(h=lens(9, 8)) == -2
        assert call(rst=18) == -2 and call(acc=20) == -2                       # misaligned: floats by 4 bytes, the fp64 sums by 8
    assert ape_call(rows=18) == -2
    bad = (ctypes.c_int32 * 8)(21, 16, 2, 1, 8, 7, 11, 10)                     # LS = 21 indexes past the J - 1 poses without the root
    assert ape_call(parts=ctypes.cast(bad, ctypes.c_void_p)) == -2
