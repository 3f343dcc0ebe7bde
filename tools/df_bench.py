"""Time the distance-field calls on the GPU (sdm_last_forward_ms; warm-up, then the median of --runs runs): Engine.distance_field, Engine.offset_mask and
Engine.outline at 1024 x 1024 and 2160 x 3840, B = 1 and 4, on four contents - `blobs` (the typical mask), a single seed pixel and a full frame (the two
extremes of an outward search), and a disk of 0.45 x the short side (the known worst case of the chunk pruning: seen from its middle every column is
about as near as the best one).  Per line: ms per call, the bytes per pixel the call must move (its inputs and outputs) and what it moves with its
intermediates (class words, carries, column distances), the implied rate of the former beside the 8 TB/s HBM peak, and the launch profile.  The last lines
give the worst / typical ratio per call and size.  usage: python tools/df_bench.py [--runs 20] [--small]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12      # bytes / s, MI355X
# bytes per pixel: (inputs + outputs, with the intermediates: 1/8 + 1/8 + 1/8 of class words written and read twice, 1/2 + 1/2 of carries, 2 + 2 of
# column distances)
BYTES = {"distance_field": (8.0, 8.0 + 5.375), "offset_mask": (8.0, 8.0 + 5.375), "outline": (32.0, 32.0 + 4.0 + 5.375)}


def content(name, B, H, W):
    import trimap_suite as TS
    if name == "blobs":
        return TS.blobs(H + W, B, H, W)
    p = np.zeros((B, H, W), np.float32)
    if name == "seed":
        p[:, H // 3, W // 3] = 1.0
    elif name == "full":
        p[:] = 1.0
    elif name == "disk":
        ys, xs = np.mgrid[0:H, 0:W]
        p[:, (ys - H // 2) ** 2 + (xs - W // 2) ** 2 <= (0.45 * min(H, W)) ** 2] = 1.0
    return p


def timed(eng, runs, call):
    for _ in range(3):
        call()
    ms = []
    for _ in range(runs):
        call()
        ms.append(eng.last_forward_ms())
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="256 x 384 only (a quick check of the tool)")
    args = ap.parse_args()
    from __graft_entry__ import load_package
    load_package()
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)
    medians = {}
    for H, W in (((256, 384), ) if args.small else ((1024, 1024), (2160, 3840))):
        for B in (1, 4):
            fg = torch.rand(B, H, W, 3, generator=torch.Generator().manual_seed(2)).cuda()
            for name in ("blobs", "seed", "full", "disk"):
                host = content(name, B, H, W)
                plane = torch.from_numpy(host).cuda()
                calls = {"distance_field": lambda: eng.distance_field(plane), "offset_mask": lambda: eng.offset_mask(plane, 40.0, 8.0),
                         "outline": lambda: eng.outline(fg, plane, 12.0, (1.0, 1.0, 1.0), "outside", 2.0)}
                if name == "seed":      # the closed form, so that the timed kernels are known to be right at this size
                    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
                    want = -((ys - H // 3) ** 2 + (xs - W // 3) ** 2)
                    want[H // 3, W // 3] = 1
                    assert np.array_equal(eng.distance_field(plane)[0].cpu().numpy(), want.astype(np.int32)), "the field is wrong"
                for call_name, call in calls.items():
                    med, lo, hi = timed(eng, args.runs, call)
                    eng.profile(True)
                    call()
                    eng.profile(False)
                    split = {k: round(v["ms"] * 1e3, 1) for k, v in eng.profile_results().items()}
                    need, moved = BYTES[call_name]
                    rate = need * B * H * W / (med * 1e-3)
                    medians[(call_name, B, H, W, name)] = med
                    print(f"[df_bench] {call_name} {B}x{H}x{W} {name}: median {med:.4f} ms (min {lo:.4f}, max {hi:.4f}); {need:.0f} B/pixel in + out "
                          f"({moved:.1f} with intermediates) = {rate / 1e9:.0f} GB/s = {100 * rate / HBM_PEAK:.1f}% of the 8 TB/s HBM peak; profile us {split}",
                          flush=True)
    for (call_name, B, H, W, name), med in sorted(medians.items()):
        if name == "blobs":
            others = {n: medians[(call_name, B, H, W, n)] for n in ("seed", "full", "disk")}
            worst = max(others, key=others.get)
            print(f"[df_bench] {call_name} {B}x{H}x{W}: worst content {worst} {others[worst]:.4f} ms / blobs {med:.4f} ms = {others[worst] / med:.2f}x "
                  f"(seed {others['seed'] / med:.2f}x, full {others['full'] / med:.2f}x, disk {others['disk'] / med:.2f}x)", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
