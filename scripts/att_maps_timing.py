#!/usr/bin/env python3
"""What the cross-attention maps cost.  Needs the GPU.

  att_maps_timing.py [OUT.json]            the maps decode (`LADiffVae.decode(return_att_maps=True)`) against the ordinary decode, and
                                           against the ordinary decode with the fused out_proj + cross-attention kernel switched off
                                           (what a maps decode runs in f16x3 mode from 4,096 rows), at 128 x 196 and 1 x 196 frames in
                                           both modes: HIP events around the call, median of 50 after 5 dropped calls, one process.
  att_maps_timing.py --child               five maps decodes per shape and mode and nothing else: the program to trace, e.g.
                                           rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/att_maps_timing.py --child
  att_maps_timing.py --decode-child        the ORDINARY decode of 128 x 196 and of 8 x 60 frames in both modes, once each, and nothing else:
                                           the program whose scripts/launch_list.py listing shows that a decode without maps makes the
                                           launches it made before.  LADIFF_LIB=<path relative to the repository> in the environment
                                           selects another build of the library (one from before the maps entry is served too).
  att_maps_timing.py --trace DIR [OUT.json]  the new kernel's own time from that trace (median over its launches per grid) and its bytes
                                           against the memory floor: per launch it reads the M = B F frame rows once (1 KiB each),
                                           the sample's folded keys G | c once per workgroup (4 T x 1028 B: the floor counts them once per
                                           sample) and writes B F T floats.

Default outputs: profiles/att_maps/timing.json and profiles/att_maps/kernel.json."""
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
SHAPES = [(128, 196), (1, 196)]
T, WARM, REPS = 5, 5, 50
HBM_TB_S = 8.0                 # MI355X HBM3E, datasheet


def floor_bytes(B, F):
    return B * F * 1024 + B * 4 * T * 1028 + B * F * T * 4


def trace(directory, out_path):
    per_grid = {}
    for f in glob.glob(directory + "/**/*kernel_trace.csv", recursive=True):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "dec_cross_maps_kernel" in r["Kernel_Name"]:
                    grid = tuple(int(r[f"Grid_Size_{a}"]) // int(r[f"Workgroup_Size_{a}"]) for a in "XY")
                    per_grid.setdefault(grid, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    if not per_grid:
        sys.exit(f"no dec_cross_maps_kernel launch in {directory}")
    result = {}
    for (B, chunks), us in sorted(per_grid.items()):
        F = dict(SHAPES).get(B)
        med, fb = float(np.median(us)), floor_bytes(B, F)
        result[f"{B}x{F}"] = {"launches": len(us), "workgroups": [B, chunks], "kernel_us_median": round(med, 2),
                              "kernel_us_min_max": [round(min(us), 2), round(max(us), 2)], "floor_bytes": fb,
                              "floor_us_at_8_TB_s": round(fb / HBM_TB_S / 1e6, 2), "GB_per_s": round(fb / med / 1e3, 1),
                              "share_of_hbm_peak": round(fb / med / 1e6 / HBM_TB_S, 3)}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(result, open(out_path, "w"), indent=1)
    print(json.dumps(result))


def main():
    import torch
    from ladiff_amd import LADiffVae, _lib, synthetic as syn
    from ladiff_amd.schema import ABL, VAE_KW
    if not torch.cuda.is_available():
        sys.exit("att_maps_timing.py measures on the GPU; none found")
    child, decode_child = "--child" in sys.argv, "--decode-child" in sys.argv
    if os.environ.get("LADIFF_LIB"):
        import ctypes
        _lib.LIB_PATH = os.path.join(ROOT, os.environ["LADIFF_LIB"])
        if not hasattr(ctypes.CDLL(_lib.LIB_PATH), "ladiff_vae_decode_att_maps"):
            _lib._SIGNATURES.pop("ladiff_vae_decode_att_maps")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "att_maps", "timing.json")
    vae = LADiffVae(ABL, **VAE_KW)
    vae.load_state_dict(syn.vae_weights(263), strict=True)
    vae = vae.cuda().eval()
    vae.graph_rows = 0
    L = _lib.lib()

    def timed(fn, warm=WARM, reps=REPS):
        times = []
        for i in range(warm + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warm:
                times.append(a.elapsed_time(b) * 1e3)
        return {"us_median": round(float(np.median(times)), 1), "us_min_max": [round(min(times), 1), round(max(times), 1)]}

    if decode_child:
        for B, F in ((128, 196), (8, 60)):
            z = torch.randn(T, B, 256, generator=torch.Generator().manual_seed(B)).cuda()
            for precision in ("fp32", "f16x3"):
                vae.precision = precision
                vae.decode(z, [F] * B)
        torch.cuda.synchronize()
        return
    result = {"T": T, "warmup": WARM, "repeats": REPS, "split_mode": _lib.split_mode_name()}
    for B, F in SHAPES:
        lens = [F] * B
        z = torch.randn(T, B, 256, generator=torch.Generator().manual_seed(B)).cuda()
        for precision in ("fp32", "f16x3"):
            vae.precision = precision
            if child:
                for _ in range(5):
                    vae.decode(z, lens, return_att_maps=True)
                torch.cuda.synchronize()
                continue
            r = {"decode": timed(lambda: vae.decode(z, lens))}
            assert L.ladiff_debug_set_decoder_fusion(1 + 64) == 0
            try:
                r["decode_out_cross_off"] = timed(lambda: vae.decode(z, lens))
            finally:
                L.ladiff_debug_set_decoder_fusion(1)
            r["decode_with_maps"] = timed(lambda: vae.decode(z, lens, return_att_maps=True))
            r["maps_over_decode"] = round(r["decode_with_maps"]["us_median"] / r["decode"]["us_median"], 3)
            r["maps_minus_out_cross_off_us"] = round(r["decode_with_maps"]["us_median"] - r["decode_out_cross_off"]["us_median"], 1)
            result[f"{B}x{F} {precision}"] = r
    if child:
        return
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(result, open(out_path, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    if "--trace" in sys.argv:
        rest = [a for a in sys.argv[1:] if not a.startswith("--")]
        trace(rest[0], rest[1] if len(rest) > 1 else os.path.join(ROOT, "profiles", "att_maps", "kernel.json"))
    else:
        main()
