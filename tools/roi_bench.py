"""Time the subject's box on the GPU (sdm_last_forward_ms; warm-up, then the median of 20 runs): Engine.subject_roi at 1080 x 1920 and 2160 x 3840,
B = 1 and 4, on a trimap whose subject sits in the middle of the frame (a quarter of the width), with the bytes of its single read (4 B H W) per second
beside the 8 TB/s HBM peak and the launch profile; Engine.refine_alpha_guided at the same sizes in the same session, as the yardstick of a
full-resolution pass; and Engine.apply_matte_roi against Engine.apply_matte_node on the same 2160 x 3840 input and inference size (synthetic weights;
--tiny: the tiny architecture at inference size 64).  usage: python tools/roi_bench.py [--runs 20] [--size 1024] [--tiny]"""
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


def centred_trimap(B, H, W):
    """Definite background outside a centred rectangle of a quarter of the width and half of the height; blobs of 0 / 0.5 / 1 inside."""
    import trimap_suite as TS
    h, w = H // 2, W // 4
    y0, x0 = (H - h) // 2, (W - w) // 2
    sub = TS.blobs(H + W, B, h, w, n=5)
    tri = np.zeros((B, H, W), np.float32)
    tri[:, y0:y0 + h, x0:x0 + w] = np.where(sub > 0.6, 1.0, np.where(sub > 0.2, 0.5, 0.0)).astype(np.float32)
    return tri


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
    ap.add_argument("--size", type=int, default=1024, help="inference size of the whole-call comparison")
    ap.add_argument("--tiny", action="store_true", help="tiny architecture for the whole-call comparison (a quick check of the tool)")
    args = ap.parse_args()
    runs = max(args.runs, 20)
    from __graft_entry__ import load_package
    load_package()
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.sdmatte_nodes import auto_subsample, subject_roi
    from comfyui_sdmatte_amd.weights import synthetic_state_dict
    eng = Engine(SDMatteConfig.tiny(), 0)
    for H, W in ((1080, 1920), (2160, 3840)):
        for B in (1, 4):
            host = centred_trimap(B, H, W)
            tri = torch.from_numpy(host).cuda()
            med, lo, hi = timed(eng, runs, lambda: eng.subject_roi(tri))
            eng.profile(True)
            got = eng.subject_roi(tri)
            eng.profile(False)
            split = {k: round(v["ms"] * 1e3, 1) for k, v in eng.profile_results().items() if k.startswith("roi_")}
            same = bool(torch.equal(got.cpu(), subject_roi(torch.from_numpy(host))))
            nbytes = 4.0 * B * H * W
            rate = nbytes / (med * 1e-3)
            red = nbytes / (split["roi_reduce"] * 1e-6)
            print(f"[roi_bench] subject_roi {B}x{H}x{W}: median {med:.4f} ms (min {lo:.4f}, max {hi:.4f}) = {rate / 1e9:.0f} GB/s of the single read = "
                  f"{100 * rate / HBM_PEAK:.1f}% of the 8 TB/s HBM peak; profile us {split} (roi_reduce alone {red / 1e9:.0f} GB/s); box {got[0].tolist()}; "
                  f"equals the CPU restatement: {same}", flush=True)
        # the yardstick: the guided refinement's full-resolution passes on the same frame (B = 1; 16 bytes per pixel each in gf_mean and gf_apply)
        g = torch.Generator().manual_seed(3)
        image = torch.rand(1, H, W, 3, generator=g).cuda()
        alpha = torch.from_numpy(centred_trimap(1, H, W)).cuda()
        s = auto_subsample(H, W, 1024)
        med, lo, hi = timed(eng, runs, lambda: eng.refine_alpha_guided(image, alpha, s))
        eng.profile(True)
        eng.refine_alpha_guided(image, alpha, s)
        eng.profile(False)
        res = eng.profile_results()
        split = {k: round(v["ms"] * 1e3, 1) for k, v in res.items() if k.startswith("gf_")}
        full = {k: (16.0 * H * W + 16.0 * (-(-H // s)) * (-(-W // s))) / (res[k]["ms"] * 1e-3) / 1e9 for k in ("gf_mean", "gf_apply")}
        print(f"[roi_bench] refine_alpha_guided 1x{H}x{W} s={s}: median {med:.4f} ms (min {lo:.4f}, max {hi:.4f}); profile us {split}; full-resolution passes "
              f"gf_mean {full['gf_mean']:.0f} GB/s, gf_apply {full['gf_apply']:.0f} GB/s", flush=True)
    eng.close()

    cfg = SDMatteConfig.tiny() if args.tiny else SDMatteConfig.full()
    S = 64 if args.tiny else args.size
    eng = Engine(cfg, 0)
    missing, _ = eng.load_state_dict(synthetic_state_dict(cfg, 0))
    assert not missing, missing[:4]
    H, W = 2160, 3840
    image = torch.rand(1, H, W, 3, generator=torch.Generator().manual_seed(4)).cuda()
    tri = torch.from_numpy(centred_trimap(1, H, W)).cuda()
    node = timed(eng, runs, lambda: eng.apply_matte_node(image, tri, S, False, "matted_rgba", True, 0.8))
    roi = timed(eng, runs, lambda: eng.apply_matte_roi(image, tri, S, False, "matted_rgba", True, 0.8))
    eng.profile(True)
    box = eng.apply_matte_roi(image, tri, S, False, "matted_rgba", True, 0.8)[3]
    eng.profile(False)
    split = {k: round(v["ms"] * 1e3, 1) for k, v in eng.profile_results().items() if k.startswith("roi_")}
    print(f"[roi_bench] 1x{H}x{W} at S={S} ({'tiny' if args.tiny else 'full'} architecture, synthetic weights): apply_matte_node median {node[0]:.3f} ms "
          f"(min {node[1]:.3f}, max {node[2]:.3f}); apply_matte_roi median {roi[0]:.3f} ms (min {roi[1]:.3f}, max {roi[2]:.3f}); box {box[0].tolist()} = "
          f"{S / box[0, 3].item():.2f} model pixels per image pixel against {S / W:.2f}; roi_ launches us {split}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
