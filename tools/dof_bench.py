"""Time Engine.defocus_background on the GPU: sdm_last_forward_ms and the per-launch times of the engine's profile (dof_prefix, dof_gather) for 16 images of
1080 x 1920 and 4 of 2160 x 3840 at radius 8 / 16 / 32 / 64, gain 0 and 4, with and without the two colour planes (warm-up, then the median of --runs
calls, with min and max), and beside each, on the same inputs and device:
  * a device-to-device copy of the call's compulsory bytes (28 per pixel without fg and bg: image 12, alpha 4, out 12; 52 with both);
  * the same call at radius 16: a cost linear in the radius gives time(64) / time(16) near 4, a per-tap gather near 16;
  * the torch restatement (sdmatte_nodes.defocus_background) on device tensors, what a user has without the kernels (--torch: it takes seconds per call
    at these sizes and radii, so it is off by default and runs at radius 8 and 16 only).
usage: python tools/dof_bench.py [--runs 10] [--sizes 16x1080x1920,4x2160x3840] [--radii 8,16,32,64] [--torch]"""
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
    ap.add_argument("--radii", default="8,16,32,64")
    ap.add_argument("--torch", action="store_true", help="also time the torch restatement on the device (radius 8 and 16)")
    args = ap.parse_args()
    from __graft_entry__ import load_package
    load_package()
    import defocus_suite as DS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.sdmatte_nodes import defocus_background
    eng = Engine(SDMatteConfig.tiny(), 0)
    radii = [int(v) for v in args.radii.split(",")]

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
        # one small scene tiled up to the size: a textured picture with a soft subject
        image, alpha, fg, bg = (torch.from_numpy(t).cuda() for t in DS.inputs("soft", 1, 1, 135, 240, planes=True))
        tile = lambda t: t.repeat(B, H // 135 + 1, W // 240 + 1, *([1] * (t.dim() - 3)))[:, :H, :W].contiguous()
        image, alpha, fg, bg = tile(image), tile(alpha), tile(fg), tile(bg)
        px = B * H * W
        copies = {False: copy_ms(px * 28 // 2), True: copy_ms(px * 52 // 2)}      # a copy of n bytes moves 2 n: read and write
        for planes in (False, True):
            f, g = (fg, bg) if planes else (None, None)
            for gain in (0.0, 4.0):
                base = median_ms(lambda: eng.defocus_background(image, alpha, f, g, 16, gain, 0.5))[0]
                for R in radii:
                    call = lambda: eng.defocus_background(image, alpha, f, g, R, gain, 0.5)
                    med, lo, hi = median_ms(call)
                    per = launches_ms(call)
                    line = (f"[dof_bench] {B}x{H}x{W} R={R} gain={gain:g} {'fg+bg' if planes else 'image only'}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) | "
                            + " ".join(f"{k} {v:.3f} ms" for k, v in per.items())
                            + f" | copy of the compulsory {52 if planes else 28} B/px {copies[planes]:.3f} ms: {med / copies[planes]:.1f} x | R=16: {base:.3f} ms, ratio {med / base:.2f}")
                    if args.torch and R <= 16:
                        out = call()
                        ref = defocus_background(image, alpha, f, g, R, gain, 0.5)
                        torch.cuda.synchronize()
                        tt = []
                        for _ in range(2):
                            t0 = time.perf_counter()
                            defocus_background(image, alpha, f, g, R, gain, 0.5)
                            torch.cuda.synchronize()
                            tt.append((time.perf_counter() - t0) * 1e3)
                        tmed = statistics.median(tt)
                        line += f" | torch restatement on the device, median wall {tmed:.1f} ms = {tmed / med:.1f} x the call; max |call - restatement| {float((out - ref).abs().max()):.2e}"
                        del out, ref
                    print(line, flush=True)
        del image, alpha, fg, bg
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
