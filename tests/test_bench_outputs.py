"""bench.py's --dump-outputs (what the last timed step returned, as float32 .npy files of at most 64 MB in all) and its argument
checks, on the CPU: the helpers the bench calls after its timed region, with stand-in outputs of the real shapes."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _outputs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, 196, 263, generator=g)
    z = torch.randn(5, B, 256, generator=g)
    return feats, z


def test_step_outputs_names_what_the_caller_receives():
    feats, z = _outputs(4)
    wl = SimpleNamespace(e2e=False, last_z=z, last_feats=None)
    assert set(bench.step_outputs(wl, feats, 1)) == {"feats", "latents"}
    assert bench.step_outputs(wl, feats, 1)["latents"][1] == 1          # prompts run along dim 1 of [max_it, B, 256]
    assert set(bench.step_outputs(wl, feats, 2)) == {"feats"}           # N > 1: the gathered frames only
    decode_only = SimpleNamespace(e2e=False, last_z=None, last_feats=None)
    assert set(bench.step_outputs(decode_only, feats, 1)) == {"feats"}
    e2e = SimpleNamespace(e2e=True, last_z=z, last_feats=feats)
    joints = torch.zeros(4, 196, 22, 3)
    assert set(bench.step_outputs(e2e, joints, 1)) == {"joints", "feats"}


def test_dump_outputs_whole_arrays_below_the_cap(tmp_path):
    feats, z = _outputs(8)
    rep = bench.dump_outputs(str(tmp_path), {"feats": (feats, 0), "latents": (z, 1)})
    assert rep["prompts"] == rep["of_prompts"] == 8 and rep["prompt_sample_seed"] is None
    f = np.load(tmp_path / "feats.npy")
    assert f.dtype == np.float32 and np.array_equal(f, feats.numpy())
    assert np.array_equal(np.load(tmp_path / "latents.npy"), z.numpy())


def test_dump_outputs_samples_the_same_prompts_of_every_array_above_the_cap(tmp_path):
    feats, z = _outputs(400)                                           # 82.5 MB + 2 MB: over the cap
    feats[:, 0, 0] = torch.arange(400, dtype=torch.float32)            # tag each prompt
    z[0, :, 0] = torch.arange(400, dtype=torch.float32)
    rep = bench.dump_outputs(str(tmp_path / "a"), {"feats": (feats, 0), "latents": (z, 1)})
    files = [tmp_path / "a" / n for n in ("feats.npy", "latents.npy")]
    assert sum(os.path.getsize(p) for p in files) <= bench.DUMP_BYTES
    assert rep["of_prompts"] == 400 and 0 < rep["prompts"] < 400 and rep["prompt_sample_seed"] == bench.DUMP_SAMPLE_SEED
    f, l = np.load(files[0]), np.load(files[1])
    rows = f[:, 0, 0].astype(int)
    assert np.array_equal(rows, l[0, :, 0].astype(int)) and np.all(np.diff(rows) > 0)
    assert np.array_equal(f, feats.numpy()[rows])
    bench.dump_outputs(str(tmp_path / "b"), {"feats": (feats, 0), "latents": (z, 1)})
    assert np.array_equal(np.load(tmp_path / "b" / "feats.npy"), f)     # the same arguments give the same sample


def test_bench_refuses_zero_timed_steps():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr and r.stdout.strip() == ""
