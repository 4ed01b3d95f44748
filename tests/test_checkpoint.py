"""Reference checkpoints into `LADIFF` (CPU): the Lightning-shaped `state_dict` of a LADiff checkpoint loads with strict=True
(`demo.py:159`), and the reference's loop-owner import (`get_model.py:12-17`) resolves to this package after
`ladiff_amd.reference_compat.install()` or under its launcher.  Nothing here touches a GPU."""
import os
import subprocess
import sys
import textwrap
from types import SimpleNamespace

import pytest
import torch

from ladiff_amd import LADIFF, MldTextEncoder, synthetic as syn
from ladiff_amd.schema import ABL, DEN_KW, VAE_KW
from conftest import ROOT

SCHED_PARAMS = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                    clip_sample=False, set_alpha_to_one=False, steps_offset=1)


def reference_cfg(t2m_path="./deps/t2m/", evaluators=True, steps=5):
    """The nodes of config_ladiff_humanml3d.yaml + base.yaml that LADIFF reads, with the reference's own dotted targets."""
    model = {"condition": "text", "guidance_scale": 7.5, "t2m_path": t2m_path,
             "denoiser": {"target": "ladiff.models.architectures.ladiff_denoiser.LADiffDenoiser", "params": {**DEN_KW, "ablation": ABL}},
             "motion_vae": {"target": "ladiff.models.architectures.ladiff_vae.LADiffVae", "params": {**VAE_KW, "ablation": ABL}},
             "scheduler": {"target": "diffusers.DDIMScheduler", "num_inference_timesteps": steps, "eta": 0.0, "params": SCHED_PARAMS}}
    if evaluators:
        model["t2m_textencoder"] = {"dim_word": 300, "dim_pos_ohot": 15, "dim_text_hidden": 512, "dim_coemb_hidden": 512}
        model["t2m_motionencoder"] = {"dim_move_hidden": 512, "dim_move_latent": 512, "dim_motion_hidden": 1024, "dim_motion_latent": 512}
    return {"model": model, "DATASET": {"NFEATS": 263, "HUMANML3D": {"UNIT_LEN": 4}}, "TEST": {"DATASETS": ["humanml3d"]},
            "TRAIN": {"ABLATION": {"MAX_IT": 5, "FRAME_PER_LATENT": 48, "TEST_EFFICIENCY": False}}}


def lightning_state_dict():
    """What `Trainer.save_checkpoint` leaves under "state_dict" for LADIFF: denoiser.*, vae.*, t2m_* - no text_encoder.* (base.py:96-104)."""
    mv, mo, tx = syn.t2m_weights(263)
    sd = {}
    for prefix, part in (("denoiser.", syn.denoiser_weights()), ("vae.", syn.vae_weights(263)), ("t2m_textencoder.", tx),
                         ("t2m_moveencoder.", mv), ("t2m_motionencoder.", mo)):
        sd.update((prefix + k, v) for k, v in part.items())
    return sd


def save_and_load(sd, path):
    torch.save({"state_dict": sd, "epoch": 3, "global_step": 1000}, path)
    return torch.load(path, map_location="cpu")["state_dict"]


def small_clip():
    return MldTextEncoder(vocab_size=1000, num_layers=1)


@pytest.fixture(scope="module")
def source():
    return lightning_state_dict()


def test_lightning_checkpoint_loads_strict(tmp_path, source):
    sd = save_and_load(source, tmp_path / "ladiff.ckpt")
    model = LADIFF(reference_cfg(t2m_path=str(tmp_path / "no_deps")), SimpleNamespace())
    result = model.load_state_dict(sd, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    mine = model.state_dict()
    assert sorted(mine) == sorted(source)
    for k, v in source.items():
        assert torch.equal(mine[k], v), k
    assert model.t2m_unit_len == 4 and model.t2m_moveencoder.input_size == 259


def test_checkpoint_with_text_encoder_keys_keeps_own_clip(tmp_path, source):
    clip = small_clip()
    gen = torch.Generator().manual_seed(5)
    for p in clip.parameters():
        p.data.copy_(torch.randn(p.shape, generator=gen))
    before = {k: v.clone() for k, v in clip.state_dict().items()}
    incoming = dict(source)
    incoming.update(("text_encoder." + k, torch.full_like(v, 7.0)) for k, v in before.items())
    incoming["text_encoder.not_a_clip_key"] = torch.zeros(3)          # dropped like every text_encoder.* key (base.py:122-125)
    model = LADIFF(reference_cfg(t2m_path=str(tmp_path)), SimpleNamespace(), text_encoder=clip)
    model.load_state_dict(save_and_load(incoming, tmp_path / "with_clip.ckpt"), strict=True)
    for k, v in clip.state_dict().items():
        assert torch.equal(v, before[k]), k
    # a model without a text encoder module drops such keys as well
    bare = LADIFF(reference_cfg(t2m_path=str(tmp_path)), SimpleNamespace(), text_encoder=lambda texts: None)
    bare.load_state_dict(incoming, strict=True)


def test_strict_still_reports_missing_and_unexpected(tmp_path, source):
    model = LADIFF(reference_cfg(t2m_path=str(tmp_path)), SimpleNamespace())
    missing = {k: v for k, v in source.items() if k != "denoiser.time_embedding.linear_1.weight"}
    assert "denoiser.time_embedding.linear_1.weight" in source
    with pytest.raises(RuntimeError, match="Missing key"):
        model.load_state_dict(missing, strict=True)
    result = model.load_state_dict(missing, strict=False)
    assert result.missing_keys == ["denoiser.time_embedding.linear_1.weight"]
    with pytest.raises(RuntimeError, match="Unexpected key"):
        model.load_state_dict({**source, "denoiser.extra": torch.zeros(1)}, strict=True)


def test_own_state_dict_round_trip(tmp_path, source):
    clip = small_clip()
    model = LADIFF(reference_cfg(t2m_path=str(tmp_path)), SimpleNamespace(), text_encoder=clip)
    model.load_state_dict(source, strict=True)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert any(k.startswith("text_encoder.") for k in before)
    model.load_state_dict(model.state_dict())
    after = model.state_dict()
    assert sorted(after) == sorted(before) and all(torch.equal(after[k], before[k]) for k in before)


def test_config_without_evaluator_nodes_builds_what_it_did(tmp_path):
    model = LADIFF(reference_cfg(evaluators=False), SimpleNamespace())
    assert not any(n.startswith("t2m_") for n, _ in model.named_children())
    sd = {k: v for k, v in lightning_state_dict().items() if not k.startswith("t2m_")}
    model.load_state_dict(sd, strict=True)


def test_evaluator_weights_from_t2m_path(tmp_path):
    """cfg.model.t2m_path/<dataset>/text_mot_match/model/finest.tar is loaded when it exists (ladiff.py:201-210)."""
    mv, mo, tx = syn.t2m_weights(263)
    d = tmp_path / "t2m" / "t2m" / "text_mot_match" / "model"
    d.mkdir(parents=True)
    torch.save({"text_encoder": tx, "movement_encoder": mv, "motion_encoder": mo}, d / "finest.tar")
    model = LADIFF(reference_cfg(t2m_path=str(tmp_path / "t2m")), SimpleNamespace())
    for k, v in tx.items():
        assert torch.equal(model.t2m_textencoder.state_dict()[k], v)
    for k, v in mo.items():
        assert torch.equal(model.t2m_motionencoder.state_dict()[k], v)


def test_range_stats_argument_errors():
    """ladiff_split_range_stats rejects bad arguments with an error code before anything reaches a GPU."""
    from ladiff_amd import _lib, build
    build.build()
    L = _lib.lib()
    assert L.ladiff_split_range_stats(None, None, -1, 0, None, None) == -1
    assert L.ladiff_split_range_stats(None, 16, 1, 4, 32, None) == -1
    assert L.ladiff_split_range_stats(16, 32, 1, -1, 64, None) == -1
    assert L.ladiff_split_range_stats(16, 32, 1, 1 << 32, 64, None) == -2
    assert L.ladiff_split_range_stats(16, 32, 65536, 4, 64, None) == -2
    assert L.ladiff_split_range_stats(None, None, 0, 0, None, None) == 0


def test_set_t2m_evaluators_overrides_children(tmp_path):
    model = LADIFF(reference_cfg(t2m_path=str(tmp_path)), SimpleNamespace())
    built = model.t2m_textencoder
    f = lambda *a: None
    model.set_t2m_evaluators(f, f, f, unit_len=5)
    assert model.t2m_textencoder is f and model.t2m_motionencoder is f and model.t2m_unit_len == 5
    assert built is not f and not any(n.startswith("t2m_") for n, _ in model.named_children())


# ---------------------------------------------------------------- the reference's import of its loop owner
GET_MODULE = textwrap.dedent("""
    import importlib, sys
    sys.path.insert(0, sys.argv[1])
    def get_module(model_type="ladiff"):                 # get_model.py:12-17
        model_module = importlib.import_module(f".modeltype.{model_type}", package="ladiff.models")
        return model_module.__getattribute__(f"{model_type.upper()}")
""")


def fake_reference(tmp_path):
    """A stand-in for the reference's package tree whose loop-owner module cannot be imported."""
    root = tmp_path / "ref"
    for d in ("ladiff", "ladiff/models", "ladiff/models/modeltype", "ladiff/models/architectures"):
        (root / d).mkdir(parents=True)
        (root / d / "__init__.py").write_text("")
    (root / "ladiff/models/modeltype/ladiff.py").write_text("raise ImportError('the reference loop owner was imported')\n")
    (root / "ladiff/models/architectures/other.py").write_text("VALUE = 'reference'\n")
    return root


def run_py(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, *args], cwd=cwd, env=env, capture_output=True, text=True, timeout=300)


def test_get_module_fails_without_install(tmp_path):
    root = fake_reference(tmp_path)
    script = tmp_path / "plain.py"
    script.write_text(GET_MODULE + "get_module()\n")
    r = run_py([str(script), str(root)], tmp_path)
    assert r.returncode != 0 and "the reference loop owner was imported" in r.stderr


def test_get_module_after_install(tmp_path):
    root = fake_reference(tmp_path)
    script = tmp_path / "installed.py"
    script.write_text(GET_MODULE + textwrap.dedent("""
        import ladiff.models.modeltype                   # the reference's packages partly imported already
        from ladiff_amd import reference_compat
        reference_compat.install()
        import ladiff_amd.pipeline
        assert get_module() is ladiff_amd.pipeline.LADIFF
        from ladiff.models.architectures import other   # every other name stays the reference's
        assert other.VALUE == "reference"
        print("OK")
    """))
    r = run_py([str(script), str(root)], tmp_path)
    assert r.returncode == 0 and "OK" in r.stdout, r.stderr


def test_launcher_runs_script_unchanged(tmp_path):
    root = fake_reference(tmp_path)
    script = tmp_path / "demo_like.py"
    script.write_text(GET_MODULE + textwrap.dedent("""
        import ladiff_amd.pipeline
        assert __name__ == "__main__"
        assert get_module() is ladiff_amd.pipeline.LADIFF
        print("ARGV", sys.argv[1:])
    """))
    r = run_py(["-m", "ladiff_amd.reference_compat", str(script), str(root), "b"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert f"ARGV {[str(root), 'b']}" in r.stdout
