"""Time Engine.refine_alpha_guided on the GPU: sdm_last_forward_ms at B = 1 for 2160 x 3840 (subsample 4), 2048^2 (subsample 2) and 1024^2 (subsample 1)
(warm-up, then the median of 20 runs), the achieved GB/s against the ideal traffic of 32 bytes per pixel (image + alpha in, image in + alpha out), the
per-kernel split from the launch profile, and beside it the same function as the torch restatement (sdmatte_nodes.guided_refine_alpha) on device
tensors - what a user has without the kernels.  usage: python tools/gf_bench.py [--runs 20] [--radius 2]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--radius", type=int, default=2)
    args = ap.parse_args()
    from __graft_entry__ import load_package
    load_package()
    import guided_suite as GS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.sdmatte_nodes import guided_refine_alpha
    eng = Engine(SDMatteConfig.tiny(), 0)
    for H, W, s in ((2160, 3840, 4), (2048, 2048, 2), (1024, 1024, 1)):
        image, alpha = GS._inputs("soft", H, 1, H, W)
        image, alpha = torch.from_numpy(image).cuda(), torch.from_numpy(alpha).cuda()
        for _ in range(3):
            out = eng.refine_alpha_guided(image, alpha, s, args.radius)
        ms = []
        for _ in range(args.runs):
            eng.refine_alpha_guided(image, alpha, s, args.radius)
            ms.append(eng.last_forward_ms())
        eng.profile(True)
        eng.refine_alpha_guided(image, alpha, s, args.radius)
        eng.profile(False)
        res = eng.profile_results()
        for _ in range(2):
            ref = guided_refine_alpha(image, alpha, s, args.radius)
        torch.cuda.synchronize()
        tt = []
        for _ in range(5):
            t0 = time.perf_counter()
            guided_refine_alpha(image, alpha, s, args.radius)
            torch.cuda.synchronize()
            tt.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ms)
        ideal = 32.0 * H * W
        split = {k: round(v["ms"], 4) for k, v in res.items() if k.startswith("gf_")}
        print(f"[gf_bench] {H}x{W} s={s} r={args.radius}: refine_alpha_guided median {med:.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}) = "
              f"{ideal / med * 1e-6:.0f} GB/s of the 32 B/pixel ideal ({ideal * 1e-6:.1f} MB); profile {split} | torch restatement on the device, median "
              f"wall {statistics.median(tt):.2f} ms; max |kernels - restatement| = {float((out - ref).abs().max()):.2e}", flush=True)
        print("\n".join(l for l in eng.profile_dump().splitlines() if l.startswith("gf_")), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
