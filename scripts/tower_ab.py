"""Same-bits A/B of the four host sequencers (vae_decode, vae_encode, clip_text_encode, denoiser_forward) and the launch-per-stage loop
between two builds of the library with one ABI: every case below runs in each library, in a child process of its own, on synthetic
weights and fixed seeds in both arithmetic modes; the outputs are dumped to .npz and compared with numpy.array_equal.  Any difference,
or a case one side lacks, is a failure (exit status 1).
usage: tower_ab.py LIB_A LIB_B [OUT_DIR]        paths relative to the repository; `product` = the shipped library
       tower_ab.py --child OUT.npz               one library (LADIFF_LIB in the environment, or the product): what a profiler wraps"""
import os, subprocess, sys
from types import SimpleNamespace
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ME = os.path.abspath(__file__)
if len(sys.argv) > 1 and sys.argv[1] != "--child":
    import numpy as np
    import tempfile
    out_dir = os.path.join(ROOT, sys.argv[3]) if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="tower_ab_")
    os.makedirs(out_dir, exist_ok=True)
    dumps = []
    for i, lib in enumerate(sys.argv[1:3]):
        env = dict(os.environ)
        if lib != "product": env["LADIFF_LIB"] = lib
        else: env.pop("LADIFF_LIB", None)
        dumps.append(os.path.join(out_dir, f"tower_ab_{i}.npz"))
        r = subprocess.run([sys.executable, ME, "--child", dumps[-1]], env=env, capture_output=True, text=True)
        print(f"{lib}: exit {r.returncode} {r.stdout.strip()[-200:]} {r.stderr.strip()[-2000:]}", flush=True)
        if r.returncode != 0: sys.exit(1)          # nothing more starts on the GPU after a failed child
    a, b = (np.load(d) for d in dumps)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in bad: print(f"MISSING on one side: {k}")
    for k in a.files:
        if k not in b.files: continue
        same = a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True) and bool(np.isfinite(a[k]).all())
        print(f"{'equal    ' if same else 'DIFFERENT'} {k}  {a[k].shape}", flush=True)
        if not same: bad.append(k)
    print(f"== {len(a.files)} outputs of {sys.argv[1]} against {sys.argv[2]}: " + ("all equal" if not bad else f"{len(bad)} FAILED: {bad}"))
    sys.exit(1 if bad else 0)

sys.path.insert(0, ROOT)
import torch
from ladiff_amd import LADIFF, DDIMScheduler, LADiffDenoiser, LADiffVae, _lib, synthetic as syn
from ladiff_amd.schema import ABL, DEN_KW, VAE_KW
from ladiff_amd.text_encoder import MldTextEncoder
if os.environ.get("LADIFF_LIB"):
    _lib.LIB_PATH = os.path.join(ROOT, os.environ["LADIFF_LIB"])
DEV = "cuda:0"
MODES = ("fp32", "f16x3")
LENS9 = [196, 60, 120, 1, 77, 196, 48, 150, 33]                           # the lists of tests/test_gpu_trained_like.py
LENS12 = LENS9 + [32, 64, 65]
L = _lib.lib()
OUT = {}


def keep(name, *tensors):
    torch.cuda.synchronize()
    for i, t in enumerate(tensors):
        OUT[f"{name} [{i}]"] = t.detach().float().cpu().numpy()


_VAE = {}
def vae(nfeats=263, T=5, fpl=48):
    if (nfeats, T, fpl) not in _VAE:
        m = LADiffVae(SimpleNamespace(**{**vars(ABL), "MAX_IT": T, "FRAME_PER_LATENT": fpl}), **{**VAE_KW, "nfeats": nfeats})
        m.load_state_dict(syn.vae_weights(nfeats, max_it=T), strict=True)
        _VAE[(nfeats, T, fpl)] = m.to(DEV).eval()
    return _VAE[(nfeats, T, fpl)]


def decode(name, mode, lens, nfeats=263, T=5, fpl=48, ragged=True, fusion=1, variant=0, graph_rows=0):
    m = vae(nfeats, T, fpl)
    z = torch.randn(T, len(lens), 256, generator=torch.Generator().manual_seed(4 + len(lens)))
    for i, l in enumerate(lens): z[-(-l // fpl):, i] = 0
    m.precision, m.length_aware, m.graph_rows = mode, ragged, graph_rows
    assert L.ladiff_debug_set_decoder_fusion(fusion) == 0 and L.ladiff_debug_set_mlp_variant(variant) == 0
    keep(f"decode {name} {mode}", m.decode(z.to(DEV), lens))
    L.ladiff_debug_set_decoder_fusion(1); L.ladiff_debug_set_mlp_variant(0)


def encode(name, mode, lens, nfeats=263, T=5, corrupt=False):
    m = vae(nfeats, T, {1: 224, 5: 48}[T])
    g = torch.Generator().manual_seed(7000 + nfeats + len(lens))
    x, eps = torch.randn(len(lens), max(lens), nfeats, generator=g), torch.randn(T, len(lens), 256, generator=g)
    c = None
    if corrupt:
        pos = torch.randperm(max(lens) * nfeats, generator=g)[:max(lens) * nfeats // 10]
        c = (pos, torch.randn(len(lens), pos.numel(), generator=g))
    m.precision = mode
    latent, dist, _ = m.encode(x.to(DEV), lens, eps=eps.to(DEV), corrupt=c)
    keep(f"encode {name} {mode}", latent, dist.loc, dist.scale)


def clip(name, mode, layers, prompts, **kw):
    enc = MldTextEncoder(vocab_size=512, num_layers=layers, precision=mode)
    enc.text_model.load_state_dict(syn.clip_weights(512, layers), strict=True)
    keep(f"clip {name} {mode}", enc.to(DEV).eval().encode_ids(syn.clip_token_ids(prompts, 512, empty_first=prompts // 2, seed=5), **kw))


def forward(den, name, mode, B2, T, masked=True, n_text=1, t=481):
    g = torch.Generator().manual_seed(1000 * B2 + 10 * T + n_text)
    x, txt = torch.randn(B2, T, 256, generator=g), torch.randn(B2, n_text, 768, generator=g)
    counts = torch.randint(1, T + 1, (B2,), generator=g).to(DEV) if masked else None
    if t is None: t = torch.randint(0, 1000, (B2,), generator=g)          # one timestep per sample
    den.precision = mode
    keep(f"forward {name} {mode}", den(x.to(DEV), torch.as_tensor(t), txt.to(DEV), max_iter_elements=counts)[0])


def loop(den, mode, use_graph):
    lens = [max(1, min(196, 48 * ((i % 5) + 1) - 5 * (i % 3))) for i in range(7)]      # latent counts 1 .. 5
    sch = DDIMScheduler(set_alpha_to_one=False, steps_offset=1, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                        beta_schedule="scaled_linear", clip_sample=False)
    pipe = LADIFF(denoiser=den, vae=vae(), scheduler=sch, guidance_scale=7.5, num_inference_timesteps=5, eta=0.0, precision=mode,
                  loop="launches", use_graph=use_graph)
    z, feats = pipe.sample(syn.text_embeddings(7, seed=907).to(DEV), lens, init_noise=syn.init_noise(lens, seed=908).to(DEV))
    pipe.check()
    keep(f"loop launches {'graphs' if use_graph else 'no graphs'} {mode}", z, feats)


with torch.no_grad():
    den = LADiffDenoiser(ABL, **DEN_KW)
    den.load_state_dict(syn.denoiser_weights(), strict=True)
    den = den.to(DEV).eval()
    for mode in MODES:
        for fusion in (0, 1, 2, 5, 9, 17, 33, 65):
            decode(f"LENS12 ragged fusion {fusion}", mode, LENS12, fusion=fusion)
            decode(f"LENS9 padded C=251 fusion {fusion}", mode, LENS9, 251, ragged=False, fusion=fusion)
        for v in range(4): decode(f"LENS12 fusion 2 mlp_variant {v}", mode, LENS12, fusion=2, variant=v)
        decode("4,905 ragged rows", mode, LENS9 * 5)
        decode("10,791 ragged rows", mode, LENS9 * 11)
        for T, fpl in ((1, 224), (3, 80), (8, 25)): decode(f"T={T} fpl={fpl}", mode, LENS9, T=T, fpl=fpl)
        decode("graphed", mode, LENS9, graph_rows=4096)
        for nfeats in (263, 251): encode(f"LENS9 C={nfeats}", mode, LENS9, nfeats)
        for B in (19, 32) + ((79, 80) if mode == "f16x3" else ()): encode(f"B={B}", mode, [LENS9[i % 9] for i in range(B)])
        encode("DVAE", mode, LENS9, corrupt=True)
        encode("S=3", mode, [1], T=1)
        clip("1 layer, 2 prompts ragged (<= 256 rows)", mode, 1, 2)
        clip("1 layer, 3 prompts padded (231 rows)", mode, 1, 3, full_length=True, dedup=False)
        clip("1 layer, 40 prompts ragged", mode, 1, 40)
        clip("1 layer, 6 prompts padded (462 rows)", mode, 1, 6, full_length=True, dedup=False)
        clip("1 layer, 107 prompts padded (8,239 rows)", mode, 1, 107, full_length=True, dedup=False)
        clip("12 layers, 4 prompts padded", mode, 12, 4, full_length=True, dedup=False)
        for B2 in (2, 43, 128):
            for T in (5, 1): forward(den, f"B2={B2} T={T}", mode, B2, T)
        forward(den, "B2=6 T=5 no mask", mode, 6, 5, masked=False)
        forward(den, "B2=7 T=5, one timestep per sample", mode, 7, 5, t=None)
        forward(den, "B2=7 T=5, one timestep per sample, no mask", mode, 7, 5, masked=False, t=None)
        for n in (2, 77): forward(den, f"B2=6 T=5, N={n} text tokens", mode, 6, 5, n_text=n)
        for use_graph in (False, True): loop(den, mode, use_graph)
import numpy as np
np.savez(sys.argv[2], **OUT)
print(f"{len(OUT)} outputs -> {sys.argv[2]}")
