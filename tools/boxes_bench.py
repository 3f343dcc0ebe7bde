"""Time a box per subject on the GPU (sdm_last_forward_ms; warm-up, then the median of 20 runs): Engine.subject_boxes with max_boxes = 4 at 1080 x 1920 and
2160 x 3840, B = 1, on a mask of three blobs with speckle, with the launch profile; beside it, in the same session, Engine.clean_mask with stage A only
(min_area = 64, no holes), which has the same labelling and is the yardstick for what the launches behind it cost; and the CPU restatement
sdmatte_nodes.subject_boxes.  Then Engine.apply_matte_boxes with N = 2, one box per image, against Engine.apply_matte_roi with B = 2 on the same frames
and inference size (synthetic weights; --tiny: the tiny architecture at inference size 64): the two differ by the sanitise launch and the paste loop.
usage: python tools/boxes_bench.py [--runs 20] [--size 1024] [--tiny] [--skip-model]"""
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


def three_subjects(H, W):
    """Three blobs of distinct sizes far apart (soft edges: trimap_suite.blobs inside each rectangle) and 400 single-pixel speckles; fp32 [1,H,W]."""
    import trimap_suite as TS
    m = np.zeros((1, H, W), np.float32)
    for i, (fy, fx, fh, fw) in enumerate(((0.10, 0.05, 0.70, 0.22), (0.30, 0.42, 0.50, 0.16), (0.55, 0.78, 0.30, 0.12))):
        y0, x0, h, w = int(fy * H), int(fx * W), int(fh * H), int(fw * W)
        sub = TS.blobs(H + i, 1, h, w, n=4)[0]
        m[0, y0:y0 + h, x0:x0 + w] = np.where(sub > 0.35, 1.0, 0.0)
    g = np.random.default_rng(9)
    m[0].ravel()[g.choice(H * W, 400, replace=False)] = 1.0
    return m


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
    ap.add_argument("--skip-model", action="store_true", help="the box timings only")
    args = ap.parse_args()
    runs = max(args.runs, 20)
    from __graft_entry__ import load_package
    load_package()
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.sdmatte_nodes import subject_boxes
    from comfyui_sdmatte_amd.weights import synthetic_state_dict
    eng = Engine(SDMatteConfig.tiny(), 0)
    for H, W in ((1080, 1920), (2160, 3840)):
        host = three_subjects(H, W)
        plane = torch.from_numpy(host).cuda()
        med, lo, hi = timed(eng, runs, lambda: eng.subject_boxes(plane, 0.0, 64, 4))
        eng.profile(True)
        got, cnt = eng.subject_boxes(plane, 0.0, 64, 4, return_count=True)
        eng.profile(False)
        split = {k: round(v["ms"] * 1e3, 1) for k, v in eng.profile_results().items()}
        t0 = time.perf_counter()
        want = subject_boxes(torch.from_numpy(host), 0.0, 64, 4)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        cm = timed(eng, runs, lambda: eng.clean_mask(plane, 0.0, 64, False, 0))
        print(f"[boxes_bench] subject_boxes 1x{H}x{W} max_boxes=4: median {med:.4f} ms (min {lo:.4f}, max {hi:.4f}); clean_mask stage A only: median "
              f"{cm[0]:.4f} ms (min {cm[1]:.4f}, max {cm[2]:.4f}); CPU restatement {cpu_ms:.0f} ms; profile us {split}; count {cnt.tolist()}, boxes "
              f"{got[0].tolist()}; equals the CPU restatement: {bool(torch.equal(got.cpu(), want))}", flush=True)
    eng.close()
    if args.skip_model:
        return

    cfg = SDMatteConfig.tiny() if args.tiny else SDMatteConfig.full()
    S = 64 if args.tiny else args.size
    eng = Engine(cfg, 0)
    missing, _ = eng.load_state_dict(synthetic_state_dict(cfg, 0))
    assert not missing, missing[:4]
    H, W = 1080, 1920
    image = torch.rand(2, H, W, 3, generator=torch.Generator().manual_seed(4)).cuda()
    host = three_subjects(H, W)
    tri = torch.from_numpy(np.concatenate([host, host[:, :, ::-1]]).copy()).cuda()
    roi = eng.subject_roi(tri)
    boxes = torch.cat([torch.arange(2, dtype=torch.int32, device=roi.device).reshape(2, 1), roi], 1).contiguous()
    by_roi = timed(eng, runs, lambda: eng.apply_matte_roi(image, tri, S, False, "matted_rgba", True, 0.8))
    by_boxes = timed(eng, runs, lambda: eng.apply_matte_boxes(image, tri, boxes, S, False, "matted_rgba", True, 0.8))
    by_roi2 = timed(eng, runs, lambda: eng.apply_matte_roi(image, tri, S, False, "matted_rgba", True, 0.8))
    eng.profile(True)
    a, m = eng.apply_matte_boxes(image, tri, boxes, S, False, "matted_rgba", True, 0.8)
    eng.profile(False)
    split = {k: round(v["ms"] * 1e3, 1) for k, v in eng.profile_results().items() if k.startswith("boxes_")}
    a2, m2, _, _ = eng.apply_matte_roi(image, tri, S, False, "matted_rgba", True, 0.8)
    print(f"[boxes_bench] 2x{H}x{W} at S={S} ({'tiny' if args.tiny else 'full'} architecture, synthetic weights): apply_matte_roi median {by_roi[0]:.3f} ms "
          f"(min {by_roi[1]:.3f}, max {by_roi[2]:.3f}), again after the other {by_roi2[0]:.3f} ms; apply_matte_boxes N=2 median {by_boxes[0]:.3f} ms (min "
          f"{by_boxes[1]:.3f}, max {by_boxes[2]:.3f}) = {100 * (by_boxes[0] / by_roi[0] - 1):+.2f}%; boxes_ launches us {split}; same bits: "
          f"{bool(torch.equal(a, a2) and torch.equal(m, m2))}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
