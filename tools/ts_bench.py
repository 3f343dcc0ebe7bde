"""Time Engine.smooth_alpha_temporal on the GPU: sdm_last_forward_ms for 16 frames of 1080 x 1920 and 8 frames of 2160 x 3840 at radius 2, patch 1
(warm-up, then the median of 20 runs), the achieved GB/s against the ideal traffic of 20 bytes per pixel and frame (image + alpha in, alpha out), and
beside it two yardsticks from the same process: a torch device-to-device copy that moves the same number of bytes (10 read + 10 written per pixel and
frame: "how far from a copy"), and the same function as the torch restatement (sdmatte_nodes.temporal_smooth_alpha) on device tensors - what a user has
without the kernel.  usage: python tools/ts_bench.py [--runs 20] [--radius 2] [--patch 1]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _event_ms(fn, runs):
    ms = []
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--patch", type=int, default=1)
    ap.add_argument("--sizes", default="16x1080x1920,8x2160x3840")
    args = ap.parse_args()
    from __graft_entry__ import load_package
    load_package()
    import temporal_suite as TS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.sdmatte_nodes import temporal_smooth_alpha
    eng = Engine(SDMatteConfig.tiny(), 0)
    for B, H, W in (tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")):
        # one small scene tiled up to the size: a static background with noise, a moving subject, a shimmering alpha
        image, _, alpha = TS.moving_disk(B, B, 135, 240)
        image = torch.from_numpy(image).cuda().repeat(1, H // 135 + 1, W // 240 + 1, 1)[:, :H, :W].contiguous()
        alpha = torch.from_numpy(alpha).cuda().repeat(1, H // 135 + 1, W // 240 + 1)[:, :H, :W].contiguous()
        for _ in range(3):
            out = eng.smooth_alpha_temporal(image, alpha, args.radius, args.patch)
        ms = []
        for _ in range(args.runs):
            eng.smooth_alpha_temporal(image, alpha, args.radius, args.patch)
            ms.append(eng.last_forward_ms())
        ideal = 20.0 * B * H * W
        src = torch.empty(int(ideal) // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        _event_ms(lambda: dst.copy_(src), 3)
        cp = _event_ms(lambda: dst.copy_(src), args.runs)
        del src, dst
        for _ in range(2):
            ref = temporal_smooth_alpha(image, alpha, args.radius, args.patch)
        torch.cuda.synchronize()
        tt = []
        for _ in range(5):
            t0 = time.perf_counter()
            temporal_smooth_alpha(image, alpha, args.radius, args.patch)
            torch.cuda.synchronize()
            tt.append((time.perf_counter() - t0) * 1e3)
        med, cmed, tmed = statistics.median(ms), statistics.median(cp), statistics.median(tt)
        print(f"[ts_bench] {B}x{H}x{W} r={args.radius} p={args.patch}: smooth_alpha_temporal median {med:.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}) = "
              f"{ideal / med * 1e-6:.0f} GB/s of the 20 B/pixel/frame ideal ({ideal * 1e-6:.1f} MB) | torch copy of the same bytes median {cmed:.4f} ms "
              f"(min {min(cp):.4f}) = {ideal / cmed * 1e-6:.0f} GB/s: the kernel takes {med / cmed:.2f} x a copy | torch restatement on the device, "
              f"median wall {tmed:.2f} ms = {tmed / med:.1f} x the kernel; max |kernel - restatement| = {float((out - ref).abs().max()):.2e}", flush=True)
        del image, alpha, out, ref
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
