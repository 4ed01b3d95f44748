"""Stage 2 (TRAIN.STAGE: diffusion) outside the sampling loop, on the CPU: the fp64 restatements of tests/diffusion_stage_ref.py against
what the reference computed for the goldens (tests/golden/make_golden_diffusion_stage.py), and the host-side plumbing - `DiffusionLosses`,
what `LADIFF` reads, the text drop's use of the numpy stream, the three new entries' declarations and argument checks.  Nothing here
calls a kernel."""
import ctypes

import numpy as np
import pytest
import torch

from ladiff_amd import LADIFF, DDIMScheduler, DDPMScheduler, DiffusionLosses, LADiffDenoiser, LADiffVae, MLDLosses, _lib, validate
from ladiff_amd.schema import ABL, DEN_KW, VAE_KW
from conftest import load_golden
from test_abi import _check_monotonic, header_functions
import diffusion_stage_ref as ref

SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False)
REF_RTOL = 1e-5                   # against the reference's fp32 pairwise sums (tests/test_vae_stage.py)
NEW = ("ladiff_denoiser_forward_timesteps_workspace_bytes", "ladiff_denoiser_forward_timesteps", "ladiff_q_sample",
       "ladiff_diffusion_losses_workspace_bytes", "ladiff_diffusion_losses")
ERR_ARG, ERR_SHAPE, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    from ladiff_amd import build
    build.build()
    return _lib.lib()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatements_equal_the_reference(tag):
    g = load_golden("diffusion_stage")
    z, noise, ts, counts = (g[f"{tag}_{k}"] for k in ("z", "noise", "timesteps", "counts"))
    want = g[f"{tag}_noisy"].numpy()
    # diffusers' fp32 arithmetic restated: the same bits
    got32 = ref.q_sample(z, noise, ts, g["alphas_cumprod"], counts, dtype=np.float32)
    assert got32.dtype == np.float32 and np.array_equal(got32, want)
    # fp64: within the reference's fp32 roundings of it (half an ulp each: the two square roots, the two products, the sum)
    got64 = ref.q_sample(z, noise, ts, g["alphas_cumprod"], counts)
    a = np.sqrt(g["alphas_cumprod"].numpy().astype(np.float64)[ts.numpy()])[:, None, None]
    mag = np.abs(a * np.transpose(z.numpy(), (1, 0, 2))) + np.abs(np.sqrt(1 - a * a) * noise.numpy())
    assert (np.abs(got64 - want) <= 3 * 2.0 ** -24 * mag + 1e-45).all()
    for i, c in enumerate(counts.tolist()):
        assert not want[i, c:].any() and want[i, :c].all() and noise[i].abs().min() > 0        # the noise keeps its padded rows
    loss, recorded = ref.inst_loss(g[f"{tag}_noise_pred"], noise), float(g[f"{tag}_inst_loss"])
    print(f"batch {tag}: inst_loss restated {loss:.9g}, reference {recorded:.9g}, relative {abs(loss - recorded) / recorded:.2e}")
    assert abs(loss - recorded) <= REF_RTOL * recorded


def test_golden_covers_what_it_says():
    g = load_golden("diffusion_stage")
    assert g["a_timesteps"].tolist() == [0, 999, 481, 481, 17, 250] and g["a_counts"].tolist() == [5, 2, 3, 1, 4, 5]
    assert g["a_z"].shape == (5, 6, 256) and g["b_z"].shape == (5, 3, 256)
    assert torch.equal(g["alphas_cumprod"], DDPMScheduler(**SCHED_KW).alphas_cumprod)


def test_diffusion_losses_interface():
    d = DiffusionLosses()
    assert d.stage == "diffusion" and d.losses == ["inst_loss", "x_loss", "total"] and d.count == 0 and d.last_batch is None
    assert d.loss2logname("total", "val") == "total/val" and d.loss2logname("inst_loss", "val") == "inst/loss/val"
    assert d.loss2logname("x_loss", "test") == "x/loss/test"
    assert set(d.compute()) == set(d.losses)
    d.add_sums({"count": 2, "sums": [3.0, 5.0]})
    d.add_sums({"count": 2, "sums": [1.0, 1.0]})
    assert d.sums()["count"] == 4 and d.sums()["sums"].tolist() == [4.0, 6.0]
    assert d.compute() == {"inst_loss": 1.0, "x_loss": 0.0, "total": 1.5}
    e = DiffusionLosses()
    e.add_sums(d)
    assert e.compute() == d.compute()
    with pytest.raises(ValueError):
        d.add_sums({"count": 1, "sums": [1.0, 2.0, 3.0, 4.0]})                  # an MLDLosses' sums
    d.reset()
    assert d.count == 0 and not d.sums()["sums"].any()
    cfg = {"TRAIN": {"STAGE": "diffusion", "ABLATION": {"PREDICT_EPSILON": True}}, "LOSS": {"LAMBDA_PRIOR": 0.0}}
    assert DiffusionLosses(True, "xyz", cfg).losses == d.losses
    with pytest.raises(NotImplementedError, match="PREDICT_EPSILON"):
        DiffusionLosses(cfg={"TRAIN": {"ABLATION": {"PREDICT_EPSILON": False}}})
    with pytest.raises(NotImplementedError, match="LAMBDA_PRIOR"):
        DiffusionLosses(cfg={"LOSS": {"LAMBDA_PRIOR": 0.5}})
    # the stage-"vae" class goes on refusing the stage, and now says where it went
    with pytest.raises(NotImplementedError, match="DiffusionLosses"):
        MLDLosses(stage="diffusion")
    with pytest.raises(NotImplementedError):
        MLDLosses(cfg={"TRAIN": {"STAGE": "diffusion"}})
    if not torch.cuda.is_available():
        with pytest.raises(_lib.LadiffHipError):
            d.update({"noise_pred": torch.zeros(2, 5, 256), "noise": torch.zeros(2, 5, 256)})
    with pytest.raises(_lib.LadiffHipError):
        d.update({"noise_pred": torch.zeros(2, 5, 256), "noise": torch.zeros(2, 4, 256)})
    with pytest.raises(_lib.LadiffHipError):
        d.update({"noise_pred": torch.zeros(2, 5, 256), "noise": 0})


def _model(**kw):
    den, vae = LADiffDenoiser(ABL, **DEN_KW), LADiffVae(ABL, **VAE_KW)
    return LADIFF(kw.pop("cfg", None), None, denoiser=den, vae=vae, scheduler=DDIMScheduler(set_alpha_to_one=False, steps_offset=1, **SCHED_KW),
                  text_encoder=kw.pop("text_encoder", lambda t: None), **kw)


def test_ladiff_reads_the_training_keys():
    m = _model()
    assert m.noise_scheduler is m.scheduler and m.guidance_uncondp == 0.1 and m.predict_epsilon is True
    ns = DDPMScheduler(**SCHED_KW)
    cfg = {"model": {"guidance_uncondp": 0.25, "noise_scheduler": {"target": "diffusers.DDPMScheduler", "params": SCHED_KW}},
           "TRAIN": {"ABLATION": {"PREDICT_EPSILON": False}}}
    m = _model(cfg=cfg)
    assert isinstance(m.noise_scheduler, DDPMScheduler) and m.noise_scheduler is not m.scheduler
    assert m.guidance_uncondp == 0.25 and m.predict_epsilon is False
    m = _model(cfg=cfg, noise_scheduler=ns, guidance_uncondp=0.5, predict_epsilon=True)      # the keywords win
    assert m.noise_scheduler is ns and m.guidance_uncondp == 0.5 and m.predict_epsilon is True
    assert torch.equal(ns.alphas_cumprod, m.scheduler.alphas_cumprod)                        # the shipped configs: one beta schedule


@pytest.mark.parametrize("cfg,key", [({"IDEA": "mld"}, "IDEA"), ({"TRAIN": {"ABLATION": {"LAD": False}}}, "LAD"),
                                     ({"TRAIN": {"ABLATION": {"PREDICT_EPSILON": False}}}, "PREDICT_EPSILON"),
                                     ({"LOSS": {"LAMBDA_PRIOR": 0.1}}, "LAMBDA_PRIOR"), ({"model": {"condition": "text_uncond"}}, "condition"),
                                     ({"TRAIN": {"SUBPHASE": "stage2"}}, "SUBPHASE"), ({"TRAIN": {"N_FRAMES": 48}}, "N_FRAMES")])
def test_other_branches_name_their_key(cfg, key):
    m = _model(cfg=cfg)
    batch = {"motion": torch.zeros(1, 8, 263), "length": [8], "text": ["a"]}
    with pytest.raises(NotImplementedError, match=key):
        m.train_diffusion_forward(batch)
    with pytest.raises(NotImplementedError, match=key):
        m._diffusion_process(torch.zeros(1, 5, 256), torch.zeros(1, 1, 768), max_iter_elements=[1])
    with pytest.raises(NotImplementedError):
        _model(cfg={"ARDIFF": True})
    _model(cfg={"IDEA": "ard", "ARDIFF": False, "TRAIN": {"SUBPHASE": "None", "N_FRAMES": "None", "ABLATION": {"LAD": True}}})._check_diffusion_branch()


class _Stop(Exception):
    pass


def test_default_text_drop_consumes_numpy_as_the_reference():
    """`"" if np.random.rand(1) < guidance_uncondp else text` per text, in order (ladiff.py:917-920): seed, call, compare which were
    blanked - and where the stream stands afterwards.  The encode is stubbed out (no GPU here); the text encoder ends the call."""
    seen = {}

    def text_encoder(texts):
        seen["texts"] = list(texts)
        raise _Stop

    m = _model(text_encoder=text_encoder, guidance_uncondp=0.4)
    m.vae.encode = lambda feats, lengths: (torch.zeros(5, len(lengths), 256), None, torch.ones(len(lengths), dtype=torch.long))
    m._check_loaded_weights = lambda: None
    texts = [f"text {i}" for i in range(40)]
    batch = {"motion": torch.zeros(40, 8, 263), "length": [8] * 40, "text": texts}
    np.random.seed(77)
    with pytest.raises(_Stop):
        m.train_diffusion_forward(batch)
    after = np.random.rand()
    np.random.seed(77)
    want = ["" if np.random.rand(1) < 0.4 else t for t in texts]
    assert seen["texts"] == want and 5 < want.count("") < 30 and len(want) == 40           # no guidance duplication
    assert after == np.random.rand()
    # drop_text replaces the draw and leaves the stream alone
    np.random.seed(78)
    with pytest.raises(_Stop):
        m.train_diffusion_forward(batch, drop_text=[i % 2 == 0 for i in range(40)])
    assert seen["texts"] == ["" if i % 2 == 0 else t for i, t in enumerate(texts)]
    np.random.seed(78)
    assert np.random.get_state()[1][:4].tolist() == np.random.RandomState(78).get_state()[1][:4].tolist()
    with pytest.raises(ValueError):
        m.train_diffusion_forward(batch, drop_text=[True])


def test_validate_picks_the_stage():
    class Model:
        cfg, is_vae = None, True

        def train_diffusion_forward(self, batch):
            raise _Stop

        def train_vae_forward(self, batch):
            raise KeyError("vae")

    with pytest.raises(_Stop):
        validate(Model(), [{}], stage="diffusion")
    with pytest.raises(_Stop):
        validate(Model(), [{}], DiffusionLosses())
    with pytest.raises(KeyError):
        validate(Model(), [{}])                                                              # the default is stage "vae", as before
    with pytest.raises(ValueError):
        validate(Model(), [{}], stage="vae_diffusion")
    out = validate(Model(), [], stage="diffusion")
    assert set(out) == {"inst_loss", "x_loss", "total"}


def test_header_binding_and_library_agree(lib):
    declared = header_functions()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.ladiff_version() == 6


def test_new_queries(lib):
    q = lib.ladiff_denoiser_forward_timesteps_workspace_bytes
    _check_monotonic("ladiff_denoiser_forward_timesteps_workspace_bytes", q, list(range(1, 301)), list(range(1, 9)))
    # O(B2 T): linear in the batch up to the carve's 256-byte rounding - never a [B2][B2 + 1] table (66 MB of c table alone at B2 = 256)
    assert q(256, 5) <= 2 * q(128, 5) and q(256, 5) - q(128, 5) < 1.01 * (q(128, 5) - q(1, 5)) * 128 / 127
    # it holds the layers' scratch of the scalar-t forward plus per-sample tables
    assert q(128, 5) >= lib.ladiff_denoiser_workspace_bytes(128, 5, 1, 1)
    ql = lib.ladiff_diffusion_losses_workspace_bytes
    _check_monotonic("ladiff_diffusion_losses_workspace_bytes", ql, [1, 3, 4, 1023, 1024, 1025, 7680, 163840, 10 ** 6, 10 ** 7, 2 ** 31 + 5])
    assert ql(1) == 8 and ql(1024) == 8 and ql(1025) == 16 and ql(2 ** 31 + 5) == 512 * 8 and ql(0) == 0


def test_argument_errors_need_no_gpu(lib):
    """Refused on the host before anything is launched: the pointers are never dereferenced (0x1000-aligned fakes)."""
    n_w = lib.ladiff_denoiser_num_params()
    w = (ctypes.c_void_p * n_w)(*([0x1000] * n_w))
    p = 0x10000
    fwd, wsb = lib.ladiff_denoiser_forward_timesteps, lib.ladiff_denoiser_forward_timesteps_workspace_bytes(6, 5)
    args = lambda **kw: [kw.get(k, d) for k, d in (("w", w), ("ws_", None), ("text", p), ("n_text", 1), ("ts", p), ("x", p), ("B2", 6), ("T", 5),
                                                    ("counts", p), ("eps", p), ("ws", p), ("wsb", wsb), ("st", None))]
    assert fwd(*args(wsb=wsb - 1)) == ERR_WORKSPACE and fwd(*args(wsb=0)) == ERR_WORKSPACE
    assert fwd(*args(T=0)) == ERR_SHAPE and fwd(*args(T=9)) == ERR_SHAPE and fwd(*args(B2=0)) == ERR_SHAPE
    assert fwd(*args(x=p + 4)) == ERR_SHAPE and fwd(*args(ts=p + 4)) == ERR_SHAPE and fwd(*args(counts=p + 2)) == ERR_SHAPE
    assert fwd(*args(n_text=2)) == ERR_UNSUPPORTED
    assert fwd(*args(ts=None)) == ERR_ARG and fwd(*args(w=None)) == ERR_ARG and fwd(*args(ws=None)) == ERR_ARG
    w_hole = (ctypes.c_void_p * n_w)(*([0x1000] * (n_w - 1) + [None]))
    assert fwd(*args(w=w_hole)) == ERR_ARG and fwd(*args(ws_=w_hole)) == ERR_ARG

    qs = lib.ladiff_q_sample
    args = lambda **kw: [kw.get(k, d) for k, d in (("z", p), ("ts", p), ("acp", p), ("n", 1000), ("counts", None), ("draw", 0), ("seed", 1),
                                                    ("first", 0), ("noise", p), ("noisy", p), ("B", 6), ("T", 5), ("st", None))]
    assert qs(*args(T=0)) == ERR_SHAPE and qs(*args(T=9)) == ERR_SHAPE and qs(*args(B=0)) == ERR_SHAPE
    assert qs(*args(z=p + 4)) == ERR_SHAPE and qs(*args(noise=p + 8)) == ERR_SHAPE and qs(*args(ts=p + 4)) == ERR_SHAPE
    assert qs(*args(noise=None)) == ERR_ARG and qs(*args(acp=None)) == ERR_ARG and qs(*args(n=0)) == ERR_ARG

    dl, n = lib.ladiff_diffusion_losses, 6 * 5 * 256
    wsb = lib.ladiff_diffusion_losses_workspace_bytes(n)
    args = lambda **kw: [kw.get(k, d) for k, d in (("pred", p), ("noise", p), ("n", n), ("lam", 1.0), ("batch", p), ("acc", p), ("ws", p),
                                                    ("wsb", wsb), ("st", None))]
    assert dl(*args(wsb=wsb - 1)) == ERR_WORKSPACE
    assert dl(*args(n=0)) == ERR_SHAPE and dl(*args(pred=p + 2)) == ERR_SHAPE and dl(*args(acc=p + 4)) == ERR_SHAPE
    assert dl(*args(ws=p + 4)) == ERR_SHAPE and dl(*args(batch=None)) == ERR_ARG
