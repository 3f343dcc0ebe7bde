"""Time the cut-out on a canvas on the GPU: Engine.compose_canvas (sdm_last_forward_ms; warm-up, then the median of the runs) against the torch restatement
sdmatte_nodes.compose_canvas on the same device (torch events around the whole function, its host readback of the box included - what a node chain
pays), at 2160 x 3840 -> 2000 x 2000 on a white background, without and with a shadow (sigma 8), 3 and 4 channels, with the launch profile and the largest
difference between the two results.  The ratio is reported, not gated.  usage: python tools/canvas_bench.py [--runs 20] [--small]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def subject(H, W):
    """A soft ellipse of half the height and a quarter of the width in the middle of the frame, random colours."""
    import canvas_suite as CS
    alpha = torch.from_numpy(CS.disc(H, W, H / 2, W / 2, H / 4, W / 8, ramp=6.0))[None]
    return torch.rand(1, H, W, 3, generator=torch.Generator().manual_seed(3)), alpha


def timed_engine(eng, runs, call):
    for _ in range(3):
        call()
    ms = []
    for _ in range(runs):
        call()
        ms.append(eng.last_forward_ms())
    return statistics.median(ms), min(ms), max(ms)


def timed_torch(runs, call):
    for _ in range(2):
        call()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="540 x 960 -> 500 x 500 (a quick check of the tool)")
    args = ap.parse_args()
    from __graft_entry__ import load_package
    load_package()
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.sdmatte_nodes import compose_canvas
    (H, W), (CH, CW) = ((540, 960), (500, 500)) if args.small else ((2160, 3840), (2000, 2000))
    fg, alpha = subject(H, W)
    fg, alpha = fg.cuda(), alpha.cuda()
    eng = Engine(SDMatteConfig.tiny(), 0)
    for shadow in (0.0, 0.5):
        for ch in (3, 4):
            kw = dict(canvas_h=CH, canvas_w=CW, fill_pct=80, valign="bottom", bg_color=(1.0, 1.0, 1.0), out_channels=ch, shadow_opacity=shadow, shadow_sigma=8.0,
                      shadow_dy=12, shadow_dx=8)
            med, lo, hi = timed_engine(eng, args.runs, lambda: eng.compose_canvas(fg, alpha, **kw))
            eng.profile(True)
            got, place = eng.compose_canvas(fg, alpha, return_placement=True, **kw)
            eng.profile(False)
            split = {k: round(v["ms"] * 1e3, 1) for k, v in eng.profile_results().items()}
            tmed, tlo, thi = timed_torch(max(3, args.runs // 4), lambda: compose_canvas(fg, alpha, **kw))
            diff = float((got - compose_canvas(fg, alpha, **kw)).abs().max())
            px = CH * CW
            print(f"[canvas_bench] 1x{H}x{W} -> {CH}x{CW}x{ch}, shadow {'on (sigma 8)' if shadow else 'off'}: compose_canvas median {med:.4f} ms (min {lo:.4f}, "
                  f"max {hi:.4f}) = {med * 1e6 / px:.3f} ns per canvas pixel; torch restatement on the device median {tmed:.3f} ms (min {tlo:.3f}, max {thi:.3f}); "
                  f"ratio {tmed / med:.1f}x; profile us {split}; placement {place[0].tolist()}; largest difference {diff:.2e}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
