"""Time Engine.estimate_foreground on the GPU: sdm_last_forward_ms at B = 1 for 1024^2, 1080 x 1920 and 2048^2 (warm-up, then the median of 20
runs), the per-kernel split from the launch profile, and beside it the same function as the torch restatement on device tensors - what a user has
without the kernels.  usage: python tools/fg_bench.py [--runs 20]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_restatement(image, alpha, reg=1e-5, gw=1.0, n_small=10, n_big=2):
    """sdmatte_nodes.estimate_foreground, but on the tensors' own device."""
    def idx(nd, ns):
        return torch.clamp((torch.arange(nd, device=image.device) * ns) // nd, max=ns - 1)

    def nb(t):
        return (torch.cat([t[:, :, :1], t[:, :, :-1]], 2), torch.cat([t[:, :, 1:], t[:, :, -1:]], 2), torch.cat([t[:, :1], t[:, :-1]], 1),
                torch.cat([t[:, 1:], t[:, -1:]], 1))
    alpha = torch.nan_to_num(alpha, nan=0.0).clamp(0.0, 1.0)
    H, W = image.shape[1:3]
    sizes = [(H, W)]
    while sizes[-1] != (1, 1):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    F = B = None
    for h, w in reversed(sizes):
        iy, ix = idx(h, H), idx(w, W)
        I, a0 = image[:, iy][:, :, ix], alpha[:, iy][:, :, ix].unsqueeze(-1)
        if F is None:
            F, B = I.clone(), I.clone()
        else:
            py, px = idx(h, F.shape[1]), idx(w, F.shape[2])
            F, B = F[:, py][:, :, px], B[:, py][:, :, px]
        a1 = 1.0 - a0
        wq = [reg + gw * (a0 - q).abs() for q in nb(a0)]
        s = wq[0] + wq[1] + wq[2] + wq[3]
        D = a0 * a0 + a1 * a1 + s
        for _ in range(n_small if max(h, w) <= 32 else n_big):
            Fq, Bq = nb(F), nb(B)
            Fm = (wq[0] * Fq[0] + wq[1] * Fq[1] + wq[2] * Fq[2] + wq[3] * Fq[3]) / s
            Bm = (wq[0] * Bq[0] + wq[1] * Bq[1] + wq[2] * Bq[2] + wq[3] * Bq[3]) / s
            r = (I - a0 * Fm - a1 * Bm) / D
            F, B = (Fm + a0 * r).clamp(0.0, 1.0), (Bm + a1 * r).clamp(0.0, 1.0)
    return F, B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    from __graft_entry__ import load_package
    load_package()
    import foreground_suite as FS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)
    for H, W in ((1024, 1024), (1080, 1920), (2048, 2048)):
        image, alpha, _, _ = FS.scene(H, 1, H, W)
        image, alpha = torch.from_numpy(image).cuda(), torch.from_numpy(alpha).cuda()
        for _ in range(3):
            eng.estimate_foreground(image, alpha)
        ms = []
        for _ in range(args.runs):
            eng.estimate_foreground(image, alpha)
            ms.append(eng.last_forward_ms())
        eng.profile(True)
        eng.estimate_foreground(image, alpha)
        eng.profile(False)
        res = eng.profile_results()
        for _ in range(2):
            torch_restatement(image, alpha)
        torch.cuda.synchronize()
        tt = []
        for _ in range(5):
            t0 = time.perf_counter()
            torch_restatement(image, alpha)
            torch.cuda.synchronize()
            tt.append((time.perf_counter() - t0) * 1e3)
        split = {k: round(v["ms"], 4) for k, v in res.items() if k.startswith("fg_")}
        print(f"[fg_bench] {H}x{W}: estimate_foreground median {statistics.median(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}) "
              f"profile {split} | torch restatement on the device, median wall {statistics.median(tt):.2f} ms", flush=True)
        print("\n".join(l for l in eng.profile_dump().splitlines() if "fg_" in l), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
