"""Time Engine.harmonize on the GPU: sdm_last_forward_ms and the per-launch times of the engine's profile (hz_stats, hz_finalize, hz_rows, hz_compose) for 16
images of 1080 x 1920 and 4 of 2160 x 3840 at sigma 2 / 6 / 16, with and without the match and the wrap (warm-up, then the median of --runs calls, with min
and max), and beside each, on the same inputs and device:
  * a device-to-device copy of the call's compulsory bytes: 40 per pixel (fg 12, alpha 4, background 12, out 12; one background per image, no fg_out);
  * the torch restatement (sdmatte_nodes.harmonize_cutout) on device tensors, what a user has without the kernels (--torch).
The streaming kernels are also given as a rate: hz_stats reads 28 bytes per pixel, hz_rows reads 16 and writes 16.
usage: python tools/hz_bench.py [--runs 10] [--sizes 16x1080x1920,4x2160x3840] [--sigmas 2,6,16] [--torch]"""
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
    ap.add_argument("--sigmas", default="2,6,16")
    ap.add_argument("--torch", action="store_true", help="also time the torch restatement on the device")
    args = ap.parse_args()
    from __graft_entry__ import load_package
    load_package()
    import harmonize_suite as HS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.sdmatte_nodes import harmonize_cutout
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

    for B, H, W in (tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")):
        # one small scene tiled up to the size: a textured subject with a soft edge over a textured scene
        fg, alpha, bg = (torch.from_numpy(t).cuda() for t in HS.inputs("soft", 1, 1, 135, 240))
        tile = lambda t: t.repeat(B, H // 135 + 1, W // 240 + 1, *([1] * (t.dim() - 3)))[:, :H, :W].contiguous()
        fg, alpha, bg = tile(fg), tile(alpha), tile(bg)
        px = B * H * W
        copy = copy_ms(px * 40 // 2)                                  # a copy of n bytes moves 2 n: read and write
        rate = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12 if ms > 0 else float("nan")
        print(f"[hz_bench] {B}x{H}x{W}: copy of the compulsory 40 B/px {copy:.3f} ms = {rate(px * 40, copy):.2f} TB/s", flush=True)
        for match, wrap in ((True, True), (True, False), (False, True), (False, False)):
            strengths = ((0.6, 0.8, 0.5) if match else (0.0, 0.0, 0.0)) + ((0.5, ) if wrap else (0.0, ))
            for sigma in (sigmas if wrap else sigmas[:1]):
                call = lambda: eng.harmonize(fg, alpha, bg, *strengths, sigma)
                med, lo, hi = median_ms(call)
                per = launches_ms(call)
                line = (f"[hz_bench] {B}x{H}x{W} match={'on' if match else 'off'} wrap={'on' if wrap else 'off'}" + (f" sigma={sigma:g}" if wrap else "")
                        + f": median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) | " + " ".join(f"{k} {v:.3f} ms" for k, v in per.items())
                        + f" | {med / copy:.2f} x the copy")
                if "hz_stats" in per:
                    line += f" | hz_stats {rate(px * 28, per['hz_stats']):.2f} TB/s"
                if "hz_rows" in per:
                    line += f" | hz_rows {rate(px * 32, per['hz_rows']):.2f} TB/s"
                if args.torch:
                    out = call()
                    ref = harmonize_cutout(fg, alpha, bg, *strengths, sigma)
                    torch.cuda.synchronize()
                    tt = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        harmonize_cutout(fg, alpha, bg, *strengths, sigma)
                        torch.cuda.synchronize()
                        tt.append((time.perf_counter() - t0) * 1e3)
                    tmed = statistics.median(tt)
                    line += f" | torch restatement on the device, median wall {tmed:.1f} ms = {tmed / med:.1f} x the call; max |call - restatement| {float((out - ref).abs().max()):.2e}"
                    del out, ref
                print(line, flush=True)
        del fg, alpha, bg
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
