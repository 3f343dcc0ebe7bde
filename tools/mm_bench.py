"""Time Engine.matte_metrics on the GPU: sdm_last_forward_ms and the per-launch times of the engine's profile for 16 images of 1080 x 1920 and 4 of
2160 x 3840 (warm-up, then the median of --runs calls, with min and max), and beside each, on the same inputs and device:
  * without Conn, at grad_sigma 0.25 / 1.4 / 4 (r = 1 / 4 / 9): a device-to-device copy that moves as many bytes as the call must read, 12 per pixel (pred, gt, trimap; the copy reads 6 and writes 6), and
    mm_pixel as a rate of those bytes;
  * with Conn: ten sdm_clean_mask(keep_largest=1, max_hole_area=0) calls on the same planes, the labelling work the call cannot avoid;
  * the torch restatement (sdmatte_nodes.matte_metrics) on device tensors, what a user has without the kernels (--torch): without Conn at the full size,
    with Conn on the first image alone (its labelling is numpy on the CPU), scaled to the batch.
usage: python tools/mm_bench.py [--runs 10] [--sizes 16x1080x1920,4x2160x3840] [--sigmas 0.25,1.4,4] [--torch]"""
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
    ap.add_argument("--sizes", default="16x1080x1920,4x2160x3840")
    ap.add_argument("--sigmas", default="0.25,1.4,4")
    ap.add_argument("--torch", action="store_true", help="also time the torch restatement on the device")
    args = ap.parse_args()
    from __graft_entry__ import load_package
    load_package()
    import metrics_suite as MS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.sdmatte_nodes import matte_metrics
    eng = Engine(SDMatteConfig.tiny(), 0)
    sigmas = [float(v) for v in args.sigmas.split(",")]

    def median_ms(fn):
        for _ in range(2):
            fn()
        ms = []
        for _ in range(args.runs):
            fn()
            ms.append(eng.last_forward_ms())
        return statistics.median(ms), min(ms), max(ms)

    def launches_ms(fn):
        eng.profile(True)
        fn()
        eng.profile(False)
        return {k: v["ms"] for k, v in eng.profile_results().items()}

    def copy_ms(nbytes):
        src = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda").normal_()
        dst = torch.empty_like(src)
        ms = []
        for i in range(args.runs + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); dst.copy_(src); e1.record(); e1.synchronize()
            if i >= 2:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    def wall_ms(fn, n=3, warm=True):
        if warm:
            fn()
        torch.cuda.synchronize()
        tt = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            tt.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(tt)

    rate = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12 if ms > 0 else float("nan")
    for B, H, W in (tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")):
        # one small scene (a soft subject, a prediction with smooth noise, a trimap with a real band) tiled up to the size
        pred, gt, tri = (torch.from_numpy(t).cuda() for t in MS._generic(3, 1, 135, 240))
        tile = lambda t: t.repeat(B, H // 135 + 1, W // 240 + 1)[:, :H, :W].contiguous()
        pred, gt, tri = tile(pred), tile(gt), tile(tri)
        px = B * H * W
        copy = copy_ms(px * 12 // 2)                                  # a copy of n bytes moves 2 n: read and write
        print(f"[mm_bench] {B}x{H}x{W}: copy that moves the compulsory 12 B/px {copy:.3f} ms = {rate(px * 12, copy):.2f} TB/s", flush=True)
        for sigma in sigmas:
            call = lambda: eng.matte_metrics(pred, gt, tri, grad_sigma=sigma, conn=False)
            med, lo, hi = median_ms(call)
            per = launches_ms(call)
            line = (f"[mm_bench] {B}x{H}x{W} conn=off sigma={sigma:g}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) | "
                    + " ".join(f"{k} {v:.3f} ms" for k, v in per.items()) + f" | {med / copy:.2f} x the copy | mm_pixel {rate(px * 12, per['mm_pixel']):.2f} TB/s")
            if args.torch:
                tmed = wall_ms(lambda: matte_metrics(pred, gt, tri, sigma, False))
                ref = matte_metrics(pred, gt, tri, sigma, False)["raw"]
                rel = float(((call()["raw"] - ref).abs() / ref.abs().clamp(min=1.0)).max())
                line += f" | torch restatement on the device, median wall {tmed:.1f} ms = {tmed / med:.1f} x the call; max relative difference of the sums {rel:.2e}"
            print(line, flush=True)
        call = lambda: eng.matte_metrics(pred, gt, tri, conn=True)
        med, lo, hi = median_ms(call)
        per = launches_ms(call)
        c = torch.minimum(pred, gt)
        one_clean = lambda k: eng.clean_mask(c, threshold=k / 10.0 - 0.05, min_area=0, keep_largest=True, max_hole_area=0)
        for k in (1, 2):
            one_clean(k)
        ten = []
        for _ in range(max(3, args.runs // 3)):
            t = 0.0
            for k in range(1, 11):
                one_clean(k)
                t += eng.last_forward_ms()
            ten.append(t)
        ten = statistics.median(ten)
        line = (f"[mm_bench] {B}x{H}x{W} conn=on sigma=1.4: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) | "
                + " ".join(f"{k} {v:.3f} ms" for k, v in per.items()) + f" | ten clean_mask(keep_largest) calls {ten:.3f} ms: the call is {med / ten:.2f} x them")
        if args.torch:
            tmed = wall_ms(lambda: matte_metrics(pred[:1], gt[:1], tri[:1], 1.4, True), n=1, warm=False) * B
            line += f" | torch restatement (labelling in numpy on the CPU), wall of one image x {B}: {tmed:.0f} ms = {tmed / med:.0f} x the call"
        print(line, flush=True)
        del pred, gt, tri, c
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
