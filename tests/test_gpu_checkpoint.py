"""Reference checkpoints on the GPU: a model loaded from a Lightning-shaped dict computes what the module-loaded model computes,
and the split operands' range check (`ladiff_split_range_stats`) gives known answers and refuses weights fp16 pairs would clip."""
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ladiff_amd import LADIFF, LADiffDenoiser, _lib, synthetic as syn
from ladiff_amd.schema import ABL, DEN_KW
from conftest import ROOT
from test_checkpoint import lightning_state_dict, reference_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENS = [60, 196, 120, 24]


def _dm():
    return SimpleNamespace(feats2joints=lambda f: f[..., :66].reshape(*f.shape[:-1], 22, 3))


def _text_encoder(seed=41):
    emb = syn.text_embeddings(len(LENS), seed=seed)                   # [2B, 1, 768], unconditional half first
    return lambda texts: emb[:len(texts)].to(DEV)


def from_checkpoint(sd, precision, tmp_path, **kw):
    model = LADIFF(reference_cfg(t2m_path=str(tmp_path)), kw.pop("dm", _dm()), text_encoder=kw.pop("text_encoder", _text_encoder()), **kw)
    model.load_state_dict(sd, strict=True)                          # demo.py:159, then .to(device), .eval()
    model.to(DEV).eval()
    model.precision = precision
    return model


def from_modules(precision, **kw):
    model = LADIFF(reference_cfg(evaluators=False), kw.pop("dm", _dm()), text_encoder=kw.pop("text_encoder", _text_encoder()), **kw)
    model.denoiser.load_state_dict(syn.denoiser_weights())
    model.vae.load_state_dict(syn.vae_weights(263))
    model.to(DEV).eval()
    model.precision = precision
    return model


def run(model):
    torch.manual_seed(7)                                           # init noise + noise seed drawn inside forward
    with torch.no_grad():
        return model({"text": ["p"] * len(LENS), "length": LENS})


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_checkpoint_model_matches_module_loaded_model(precision, tmp_path):
    ck = from_checkpoint(lightning_state_dict(), precision, tmp_path)
    ref = from_modules(precision)
    a, b = run(ck), run(ref)
    assert [tuple(j.shape) for j in a] == [(l, 22, 3) for l in LENS]
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert ck._range_check_pending == (not _lib.is_split(precision))   # the check ran (split) or is still owed (fp32)


def test_t2m_eval_with_checkpoint_evaluators(tmp_path):
    from test_gpu_evaluators import make_evaluators
    rs = np.random.RandomState(2)
    mean = torch.from_numpy(rs.standard_normal(263).astype(np.float32)) * 0.1
    std = torch.from_numpy(rs.uniform(0.5, 1.5, 263).astype(np.float32))
    dm = SimpleNamespace(renorm4t2m=lambda f: (f - mean.to(f.device)) / std.to(f.device), feats2joints=_dm().feats2joints)
    B = len(LENS)
    gen = torch.Generator().manual_seed(63)
    motions = torch.randn(B, max(LENS), 263, generator=gen)
    word = torch.randn(B, 12, 300, generator=gen)
    pos = torch.nn.functional.one_hot(torch.randint(0, 15, (B, 12), generator=gen), 15).float()
    batch = {"text": ["a"] * B, "length": LENS, "motion": motions, "word_embs": word, "pos_ohot": pos, "text_len": torch.tensor([12, 9, 7, 3])}
    ck = from_checkpoint(lightning_state_dict(), "f16x3", tmp_path, dm=dm)
    ref = from_modules("f16x3", dm=dm)
    move, motion, text = make_evaluators(263)
    ref.set_t2m_evaluators(text, move, motion, unit_len=4)
    torch.manual_seed(9)
    a = ck.t2m_eval(batch)
    torch.manual_seed(9)
    b = ref.t2m_eval(batch)
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------- the range kernel against a restatement of the conversion
def rtz_f16(x):
    """fp32 -> fp16 rounded toward zero, saturating at +-65504 (v_cvt_pkrtz_f16_f32 on finite input)."""
    xc = np.clip(x, -65504.0, 65504.0).astype(np.float32)
    h = xc.astype(np.float16)                                       # round to nearest even ...
    over = np.abs(h.astype(np.float32)) > np.abs(xc)
    h[over] = np.nextafter(h[over], np.float16(0))                  # ... one step back toward zero where it rounded away
    return h.astype(np.float32)


def expected_stats(x):
    x = np.asarray(x, dtype=np.float32)
    fin = np.isfinite(x)
    xf = x[fin]
    hi = rtz_f16(xf)
    lo = rtz_f16((xf - hi).astype(np.float32))
    err = np.abs((xf - hi).astype(np.float32) - lo).astype(np.float32)
    ax = np.abs(xf)
    nonnan = np.abs(x[~np.isnan(x)])
    return {"numel": x.size, "max_abs": float(nonnan.max()) if nonnan.size else 0.0, "max_err": float(err.max()) if err.size else 0.0,
            "nonfinite": int((~fin).sum()), "beyond_range": int((ax > 65504).sum()),
            "coarse": int(((ax != 0) & (err > ax * np.float32(2.0 ** -11))).sum())}, xf, err


def case(n, seed):
    rs = np.random.RandomState(seed)
    mag = 2.0 ** rs.uniform(-30, 17.5, n)                          # 2^-30 .. ~185000: subnormal lo, exact range, saturation
    x = (mag * rs.choice([-1.0, 1.0], n)).astype(np.float32)
    if n >= 16:
        x[:9] = [0.0, np.inf, -np.inf, np.nan, 2e5, -65504.0, 65505.0, 131008.0, 1e-30]
        rs.shuffle(x)
    return x


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 4 * 1023 + 1, 3 * (1 << 20) + 7])
def test_range_kernel_known_answers(n):
    assert _lib.split_mode_name() == "f16x3"
    xs = [case(n, 100 + n), np.array([2e5] * min(n, 3), dtype=np.float32), np.full(n, 0.75, dtype=np.float32)]
    got = _lib.split_range_stats([torch.from_numpy(x).to(DEV) for x in xs])
    for x, g in zip(xs, got):
        want, xf, err = expected_stats(x)
        assert g == want
        inside = np.abs(xf) <= 65504
        assert (err[inside] <= np.maximum(2.0 ** -20 * np.abs(xf[inside]), 2.0 ** -24)).all()


def test_range_kernel_unaligned_tensor():
    x = case(4 * 257 + 3, 5)
    base = torch.from_numpy(x).to(DEV)
    view = base[1:]                                                # 4 bytes past a 16-byte boundary: the scalar pass
    assert view.data_ptr() % 16 == 4
    table = torch.tensor([view.data_ptr(), view.numel()], dtype=torch.int64, device=DEV)
    stats = torch.empty(1, 5, dtype=torch.int64, device=DEV)
    L = _lib.lib()
    _lib.check(L.ladiff_split_range_stats(table.data_ptr(), table.data_ptr() + 8, 1, view.numel(), stats.data_ptr(), _lib.stream_ptr()))
    h = stats.cpu().numpy()
    want, _, _ = expected_stats(x[1:])
    assert h[0, 0:2].astype(np.uint32).view(np.float32).tolist() == [want["max_abs"], want["max_err"]]
    assert h[0, 2:].tolist() == [want["nonfinite"], want["beyond_range"], want["coarse"]]


def test_synthetic_denoiser_table_in_range():
    den = LADiffDenoiser(ABL, **DEN_KW)
    den.load_state_dict(syn.denoiser_weights())
    table = den.to(DEV)._weight_table()
    report = table.range_report()
    split = [n for n, t in zip(table.names, table.tensors) if t.dim() == 2 and t.shape[1] % 64 == 0]
    assert sorted(report) == sorted(split) and len(report) > 50
    assert all(st["beyond_range"] == 0 and st["nonfinite"] == 0 for st in report.values())
    assert max(st["max_abs"] for st in report.values()) < 65504


# ---------------------------------------------------------------- refusal on the checkpoint path
BAD_KEY = "denoiser.time_embedding.linear_1.weight"


def test_out_of_range_checkpoint_weight_is_refused_in_split_mode(tmp_path):
    sd = lightning_state_dict()
    sd[BAD_KEY] = sd[BAD_KEY].clone()
    sd[BAD_KEY][3, 5] = 2e5
    model = from_checkpoint(sd, "f16x3", tmp_path)
    with pytest.raises(_lib.LadiffHipError, match=BAD_KEY.replace(".", r"\.")) as e:
        run(model)
    assert "select_split_format" in str(e.value)
    assert model._call == 0 and not model._plans and not model.times  # nothing of the call was launched
    with pytest.raises(_lib.LadiffHipError):
        run(model)                                                  # still refused: the check is owed until it passes
    model.precision = "fp32"
    assert len(run(model)) == len(LENS)                             # fp32 operands: no pairs, no refusal
    stats = dict(model.check_split_range())                         # the report itself, in fp32 mode: no raise
    assert stats[BAD_KEY]["beyond_range"] == 1 and stats[BAD_KEY]["max_abs"] == 2e5

    # the same weights given at module level keep today's behaviour: no check, the call runs
    plain = from_modules("f16x3")
    plain.denoiser.load_state_dict({k[len("denoiser."):]: v for k, v in sd.items() if k.startswith("denoiser.")})
    assert len(run(plain)) == len(LENS) and not plain._range_check_pending


def test_bf16_flavour_has_no_beyond_range():
    """bf16 halves keep fp32's exponent range: the same 2e5 value is not beyond it (child process: one format per process)."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import torch\n"
            "from ladiff_amd import _lib\n"
            "_lib.select_split_format('bf16')\n"
            "st = _lib.split_range_stats([torch.tensor([2e5, -3.0, 65505.0, 1.0], device='cuda:0')])[0]\n"
            "assert _lib.split_mode_name() == 'bf16x3'\n"
            "assert st['beyond_range'] == 0 and st['nonfinite'] == 0 and st['max_abs'] == 2e5, st\n"
            "print('OK')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stderr
