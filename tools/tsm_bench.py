"""Time Engine.smooth_alpha_motion on the GPU: sdm_last_forward_ms for 16 frames of 1080 x 1920 and 8 frames of 2160 x 3840 at radius 2, patch 1,
search 2 / 4 / 8 and at radius 4, patch 2, search 4 (warm-up, then the median of --runs calls), and beside it, on the same inputs and device: ts_smooth
(Engine.smooth_alpha_temporal at the same radius and patch) with the ratio next to (2 search + 1)^2 - the cost of evaluating every candidate with the
existing arithmetic and no sharing, so a ratio above it means the sharing is not working - and the torch restatement
(sdmatte_nodes.temporal_smooth_alpha_motion) on device tensors, what a user has without the kernel.
usage: python tools/tsm_bench.py [--runs 10] [--sizes 16x1080x1920,8x2160x3840] [--configs 2:1:2,2:1:4,2:1:8,4:2:4] [--no-torch]"""
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
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--sizes", default="16x1080x1920,8x2160x3840")
    ap.add_argument("--configs", default="2:1:2,2:1:4,2:1:8,4:2:4", help="radius:patch:search, comma-separated")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch restatement (it takes seconds per call at these sizes)")
    args = ap.parse_args()
    from __graft_entry__ import load_package
    load_package()
    import temporal_suite as TS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.sdmatte_nodes import temporal_smooth_alpha_motion
    eng = Engine(SDMatteConfig.tiny(), 0)

    def median_ms(fn):
        for _ in range(2):
            out = fn()
        ms = []
        for _ in range(args.runs):
            fn()
            ms.append(eng.last_forward_ms())
        return statistics.median(ms), min(ms), max(ms), out

    for B, H, W in (tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")):
        # one small scene tiled up to the size: a static background with noise, a subject moving 2 pixels per frame, a shimmering alpha
        image, _, alpha = TS.moving_disk(B, B, 135, 240, speed=2.0)
        image = torch.from_numpy(image).cuda().repeat(1, H // 135 + 1, W // 240 + 1, 1)[:, :H, :W].contiguous()
        alpha = torch.from_numpy(alpha).cuda().repeat(1, H // 135 + 1, W // 240 + 1)[:, :H, :W].contiguous()
        for radius, patch, search in (tuple(int(v) for v in c.split(":")) for c in args.configs.split(",")):
            med, lo, hi, out = median_ms(lambda: eng.smooth_alpha_motion(image, alpha, radius, patch, search))
            ts, _, _, _ = median_ms(lambda: eng.smooth_alpha_temporal(image, alpha, radius, patch))
            line = (f"[tsm_bench] {B}x{H}x{W} r={radius} p={patch} s={search}: smooth_alpha_motion median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) | "
                    f"ts_smooth on the same input {ts:.4f} ms: ratio {med / ts:.1f} against (2 s + 1)^2 = {(2 * search + 1) ** 2}")
            if not args.no_torch:
                ref = temporal_smooth_alpha_motion(image, alpha, radius, patch, search)
                torch.cuda.synchronize()
                tt = []
                for _ in range(2):
                    t0 = time.perf_counter()
                    temporal_smooth_alpha_motion(image, alpha, radius, patch, search)
                    torch.cuda.synchronize()
                    tt.append((time.perf_counter() - t0) * 1e3)
                tmed = statistics.median(tt)
                diff = (out - ref).abs()
                line += (f" | torch restatement on the device, median wall {tmed:.1f} ms = {tmed / med:.1f} x the kernel; |kernel - restatement| > 1e-5 on "
                         f"{float((diff > 1e-5).float().mean()) * 100:.4f} % of the pixels (near-ties of the choice)")
                del ref, diff
            print(line, flush=True)
            del out
        del image, alpha
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
