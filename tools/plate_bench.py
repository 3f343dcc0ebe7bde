"""Time Engine.fill_background on the GPU: sdm_last_forward_ms and the time of every launch from the engine's profile (plate_pull ..., plate_small,
plate_push ...) for 16 images of 1080 x 1920 and 4 of 2160 x 3840, on the image alone and with the bg and hole planes (warm-up, then the median of --runs
calls, with min and max), and beside each, on the same inputs and device:
  * a device-to-device copy of the call's compulsory bytes (28 per pixel: C 12, alpha 4, out 12; 32 with the hole plane);
  * the bytes the design moves (the engine's own count per launch: level 0 is read by the first pull and again by the last push, the pyramid is
    written and read once) and the rate each launch reaches on them;
  * the torch restatement (sdmatte_nodes.clean_plate) on device tensors, what a user has without the kernels (--no-torch to skip).
usage: python tools/plate_bench.py [--runs 10] [--sizes 16x1080x1920,4x2160x3840] [--no-torch]"""
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
    ap.add_argument("--no-torch", action="store_true", help="skip the torch restatement on the device")
    args = ap.parse_args()
    from __graft_entry__ import load_package
    load_package()
    import plate_suite as PS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.sdmatte_nodes import clean_plate
    eng = Engine(SDMatteConfig.tiny(), 0)

    def median_ms(fn):
        for _ in range(2):
            fn()
        ms = []
        for _ in range(args.runs):
            fn()
            ms.append(eng.last_forward_ms())
        return statistics.median(ms), min(ms), max(ms)

    def launches(fn):
        """[(name, ms, MB)] in launch order, the median over --runs profiled calls of each launch's time"""
        runs = []
        for _ in range(args.runs):
            eng.profile(True)
            fn()
            eng.profile(False)
            rows = [line.split(",") for line in eng.profile_dump().strip().split("\n")[1:]]
            runs.append([(r[0], float(r[1]), float(r[3])) for r in rows])
        return [(runs[0][i][0], statistics.median(r[i][1] for r in runs), runs[0][i][2]) for i in range(len(runs[0]))]

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
        # one small scene tiled up to the size: a textured picture with a soft subject and a second object
        image, alpha, bg, hole = (torch.from_numpy(t).cuda() for t in PS.inputs("soft", 1, 1, 135, 240, with_bg=True, with_hole=True))
        tile = lambda t: t.repeat(B, H // 135 + 1, W // 240 + 1, *([1] * (t.dim() - 3)))[:, :H, :W].contiguous()
        image, alpha, bg, hole = tile(image), tile(alpha), tile(bg), tile(hole)
        px = B * H * W
        assert sum(eng.plate_launches(H, W)) == sum(PS.launches(H, W).values())
        for planes in (False, True):
            g, h, cut = (bg, hole, 1.0) if planes else (None, None, PS.ALPHA_CUT)
            bpp = 32 if planes else 28
            copy = copy_ms(px * bpp // 2)                                   # a copy of n bytes moves 2 n: read and write
            call = lambda: eng.fill_background(image, alpha, g, h, cut)
            med, lo, hi = median_ms(call)
            per = launches(call)
            moved = sum(mb for _, _, mb in per)
            line = (f"[plate_bench] {B}x{H}x{W} {'bg + hole, cut 1' if planes else 'image only, cut 1/16'}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}), "
                    f"{len(per)} launches | " + " ".join(f"{k} {ms:.3f} ms ({mb / ms:.0f} GB/s)" for k, ms, mb in per)
                    + f" | copy of the compulsory {bpp} B/px {copy:.3f} ms: {med / copy:.2f} x | designed traffic {moved / px * 1e6:.1f} B/px = "
                    f"{moved * 1e6 / (px * bpp):.2f} x the compulsory")
            if not args.no_torch:
                out = call()
                ref = clean_plate(image, alpha, g, h, cut)
                torch.cuda.synchronize()
                tt = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    clean_plate(image, alpha, g, h, cut)
                    torch.cuda.synchronize()
                    tt.append((time.perf_counter() - t0) * 1e3)
                tmed = statistics.median(tt)
                line += f" | torch restatement on the device, median wall {tmed:.1f} ms = {tmed / med:.1f} x the call; max |call - restatement| {float((out - ref).abs().max()):.2e}"
                del out, ref
            print(line, flush=True)
        del image, alpha, bg, hole
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
