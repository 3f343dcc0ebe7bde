"""Time the green-screen calls on the GPU: sdm_last_forward_ms and the per-launch times of the engine's profile for 16 images of 1080 x 1920 and 4 of
2160 x 3840 (warm-up, then the median of --runs calls, with min and max):
  * Engine.screen_colour on `screen`-like content (most pixels in a few bins: the wave's one-bin path of ck_hist) and on `noise` (every bin: one LDS
    atomic per pixel), per image and shared - the two ends of the histogram's conflict behaviour;
  * Engine.chroma_key with each output set, against a colour and against a plane;
  * Engine.key_screen, one pass and two.
Beside each, on the same device: a device-to-device copy of the call's compulsory bytes (the colour reads the image twice: 24 per pixel; the key reads 12,
or 24 with a plane, and writes 4 per plane and 12 for the despilled image), and with --torch the torch restatement on device tensors, what a user has
without the kernels.  ck_hist, ck_mean and ck_key are also given as a rate.
usage: python tools/ck_bench.py [--runs 10] [--sizes 16x1080x1920,4x2160x3840] [--torch]"""
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
    ap.add_argument("--torch", action="store_true", help="also time the torch restatement on the device")
    args = ap.parse_args()
    from __graft_entry__ import load_package
    load_package()
    import key_suite as KS
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)

    def median_ms(fn):
        for _ in range(2):
            fn()
        ms = []
        for _ in range(args.runs):
            fn()
            ms.append(eng.last_forward_ms())
        return statistics.median(ms), min(ms), max(ms)

    def chain_ms(fn):
        """several engine calls in one: events on torch's current stream around the whole chain"""
        ms = []
        for i in range(args.runs + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            if i >= 2:
                ms.append(e0.elapsed_time(e1))
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

    def torch_ms(fn):
        fn()
        torch.cuda.synchronize()
        tt = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            tt.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(tt)

    rate = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12 if ms > 0 else float("nan")
    for B, H, W in (tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")):
        px = B * H * W
        tile = lambda t: t.repeat(B, H // 135 + 1, W // 240 + 1, 1)[:, :H, :W].contiguous()
        contents = {"screen": tile(torch.from_numpy(KS.inputs("screen", 1, 1, 135, 240)).cuda()), "noise": torch.rand(B, H, W, 3, device="cuda")}
        copies = {n: copy_ms(px * n // 2) for n in (16, 24, 28, 32, 40)}      # a copy of n bytes moves 2 n: read and write
        print(f"[ck_bench] {B}x{H}x{W}: copy of 24 B/px {copies[24]:.3f} ms = {rate(px * 24, copies[24]):.2f} TB/s", flush=True)
        for content, img in contents.items():
            for share in (False, True):
                call = lambda: eng.screen_colour(img, "any" if content == "noise" else "green", share)
                med, lo, hi = median_ms(call)
                per = launches_ms(call)
                line = (f"[ck_bench] {B}x{H}x{W} screen_colour {content} share={int(share)}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) | "
                        + " ".join(f"{k} {v:.3f} ms" for k, v in per.items()) + f" | {med / copies[24]:.2f} x the copy of 24 B/px"
                        + f" | ck_hist {rate(px * 12, per['ck_hist']):.2f} TB/s ck_mean {rate(px * 12, per['ck_mean']):.2f} TB/s")
                if args.torch and not share:
                    tm = torch_ms(lambda: N.screen_colour(img, "any" if content == "noise" else "green", share))
                    line += f" | torch restatement on the device, median wall {tm:.1f} ms = {tm / med:.1f} x the call"
                print(line, flush=True)
        img = contents["screen"]
        colour = eng.screen_colour(img, "green")
        plane = eng.fill_background(img, eng.chroma_key(img, colour, want="key"), alpha_cut=0.25)
        for screen, sname in ((colour, "colour"), (plane, "plane")):
            for want in (("key", ), ("despilled", ), ("key", "despilled"), ("trimap", ), KS.OUTPUTS):
                nbytes = (12 if sname == "colour" else 24) + sum({"key": 4, "trimap": 4, "despilled": 12}[w] for w in want)
                call = lambda: eng.chroma_key(img, screen, want=want)
                med, lo, hi = median_ms(call)
                per = launches_ms(call)
                cp = copies[min(copies, key=lambda n: abs(n - nbytes))] * nbytes / min(copies, key=lambda n: abs(n - nbytes))
                kbytes = nbytes - (4 if "trimap" in want else 0) + (1 if "trimap" in want else 0) + (4 if want == ("trimap", ) else 0)
                line = (f"[ck_bench] {B}x{H}x{W} chroma_key {sname} want={'+'.join(want)}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) | "
                        + " ".join(f"{k} {v:.3f} ms" for k, v in per.items()) + f" | {med / cp:.2f} x a copy of its {nbytes} B/px"
                        + f" | ck_key {rate(px * kbytes, per['ck_key']):.2f} TB/s")
                if args.torch and want == ("key", "despilled"):      # (the restatement's trimap runs on the CPU)
                    tm = torch_ms(lambda: N.chroma_key(img, screen, want=want))
                    line += f" | torch restatement, median wall {tm:.1f} ms = {tm / med:.1f} x the call"
                print(line, flush=True)
        for correction in (False, True):
            med, lo, hi = chain_ms(lambda: eng.key_screen(img, "green", False, correction, sync=False))
            print(f"[ck_bench] {B}x{H}x{W} key_screen screen_correction={int(correction)}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
        del contents, img, colour, plane
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
