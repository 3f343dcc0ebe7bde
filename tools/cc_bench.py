"""Time Engine.clean_mask on the GPU: sdm_last_forward_ms at B = 1 for 1080 x 1920 and 2160 x 3840 with both stages on (warm-up, then the median of
20 runs), on a blob mask with speckle and on the serpentine (one line through every tile seam: the long-chain case of the union-find), the per-kernel
split from the launch profile, the fraction of the HBM peak the 64 bytes per pixel of the ten launches amount to, and beside it what a user runs
without the kernels: the host labelling (scipy.ndimage.label where importable, otherwise the reference of tests/cleanmask_suite.py) plus the two
copies of the mask between device and host.  usage: python tools/cc_bench.py [--runs 20]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# bytes per pixel: stage A tile 12 (mask in, label and area out), flatten 8, select 2 x 4, apply 12; stage B tile 12, flatten 8, fill 4
BYTES_PER_PIXEL = 12 + 8 + 8 + 12 + 12 + 8 + 4
HBM_PEAK = 8.0e12      # bytes / s, MI355X


def host_clean(mask, min_area, max_hole_area):
    """The host version a pipeline has today: two scipy labellings and bincounts (or the suite's reference), on a numpy mask."""
    try:
        from scipy import ndimage as ndi
    except ImportError:
        import cleanmask_suite as CS
        return "suite reference", CS.reference(mask, 0.5, min_area, False, max_hole_area, False)[0]
    out = mask.copy()
    for b in range(mask.shape[0]):
        fg = mask[b] > 0.5
        lab, _ = ndi.label(fg, structure=np.ones((3, 3), int))
        keep = (np.bincount(lab.ravel()) >= min_area)
        keep[0] = False
        keep = keep[lab]
        lab, n = ndi.label(~keep)
        area = np.bincount(lab.ravel(), minlength=n + 1)
        edge = np.zeros(n + 1, bool)
        for line in (lab[0], lab[-1], lab[:, 0], lab[:, -1]):
            edge[line] = True
        fill = (~edge & (area <= max_hole_area))
        fill[0] = False
        out[b][fg & ~keep] = 0.0
        out[b][fill[lab]] = 1.0
    return "scipy.ndimage.label", out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    from __graft_entry__ import load_package
    load_package()
    import cleanmask_suite as CS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)
    for H, W in ((1080, 1920), (2160, 3840)):
        for name, host in (("blobs", CS.blobs(H, 1, H, W, n=9)), ("serpentine", CS._serpentine(1, H, W))):
            mask = torch.from_numpy(host).cuda()
            for _ in range(3):
                eng.clean_mask(mask, 0.5, 64, False, 64)
            ms = []
            for _ in range(args.runs):
                eng.clean_mask(mask, 0.5, 64, False, 64)
                ms.append(eng.last_forward_ms())
            eng.profile(True)
            got = eng.clean_mask(mask, 0.5, 64, False, 64)
            eng.profile(False)
            split = {k: round(v["ms"], 4) for k, v in eng.profile_results().items() if k.startswith("cc_")}
            tt = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                how, want = host_clean(mask.cpu().numpy(), 64, 64)
                back = torch.from_numpy(want).cuda()
                torch.cuda.synchronize()
                tt.append((time.perf_counter() - t0) * 1e3)
            same = bool(torch.equal(back, got))
            med = statistics.median(ms)
            frac = BYTES_PER_PIXEL * H * W / (med * 1e-3) / HBM_PEAK
            print(f"[cc_bench] {H}x{W} {name}: clean_mask median {med:.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}) = {BYTES_PER_PIXEL} B/pixel at "
                  f"{100 * frac:.1f}% of the HBM peak; profile {split} | {how} on the host + 2 copies, median wall {statistics.median(tt):.1f} ms; "
                  f"same result: {same}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
