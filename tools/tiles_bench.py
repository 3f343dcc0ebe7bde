"""Time the tiled matting calls on the GPU at 2160 x 3840, B = 1, on a synthetic trimap whose unknown band is a ring (a portrait-sized subject), with the tiny
architecture so that the model does not drown the new kernels (warm-up, then the median of --runs calls, with min and max):
  * Engine.band_tiles: sdm_last_forward_ms and the per-launch times of the engine's profile, beside a device-to-device copy that moves the compulsory
    4 B/px (the one read of the plane), and the torch restatement of the same rule on the same device;
  * tiles_blend alone, from the per-launch profile of Engine.apply_matte_tiles, beside a copy that moves its compulsory 8 B/px (the write, and a base or slot
    value per pixel), and the torch restatement of the blend (sdmatte_nodes.blend_tiles' arithmetic on device tensors);
  * the number of active tiles against the grid cells.
usage: python tools/tiles_bench.py [--runs 10] [--size 2160x3840] [--tile 1024] [--overlap 128] [--feather 128] [--S 64,256]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_band_tiles(trimap, lo, hi, oy, sy, ox, sx):
    """The active cells of image 0 by the rule, on the tensor's device: a list of (y0, x0)."""
    band = (trimap[0] > lo) & (trimap[0] < hi)
    flags = torch.stack([band[y0:y0 + sy, x0:x0 + sx].any() for y0 in oy for x0 in ox]).cpu().tolist()
    return [(y0, x0) for (y0, x0), f in zip(((y0, x0) for y0 in oy for x0 in ox), flags) if f]


def torch_blend(crops, tiles, trimap, feather):
    """sdmatte_nodes.blend_tiles' arithmetic on device tensors (B = 1, the definite trimap as the base)."""
    from comfyui_sdmatte_amd.sdmatte_nodes import _tile_axis_weight
    _, H, W = trimap.shape
    dev = trimap.device
    wsum, acc, ws = torch.zeros(H, W, device=dev), torch.zeros(H, W, device=dev), []
    for _, y0, x0, h, w in tiles:
        wn = _tile_axis_weight(y0, h, H, feather).to(dev)[:, None] * _tile_axis_weight(x0, w, W, feather).to(dev)[None, :]
        ws.append(wn)
        wsum[y0:y0 + h, x0:x0 + w] += wn
    for (_, y0, x0, h, w), wn, crop in zip(tiles, ws, crops):
        acc[y0:y0 + h, x0:x0 + w] += (wn / wsum[y0:y0 + h, x0:x0 + w]) * crop
    return torch.where(wsum > 0, acc.clamp(0, 1), (trimap[0] > 0.5).float())[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--size", default="2160x3840")
    ap.add_argument("--tile", type=int, default=1024)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--feather", type=int, default=128)
    ap.add_argument("--S", default="64,256", help="inference sizes of the tiny model (the blend resamples a slot of S x S to the tile)")
    args = ap.parse_args()
    from __graft_entry__ import load_package
    load_package()
    import tiles_suite as TS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.sdmatte_nodes import compact_boxes, tile_axis
    from comfyui_sdmatte_amd.weights import synthetic_state_dict
    cfg = SDMatteConfig.tiny()
    eng = Engine(cfg, 0)
    eng.load_state_dict(synthetic_state_dict(cfg, 0))
    H, W = (int(v) for v in args.size.split("x"))
    px = H * W

    def median_ms(fn):
        for _ in range(2):
            fn()
        ms = []
        for _ in range(args.runs):
            fn()
            ms.append(eng.last_forward_ms())
        return statistics.median(ms), min(ms), max(ms)

    def launches_ms(fn, runs=1):
        out = {}
        for _ in range(runs):
            eng.profile(True)
            fn()
            eng.profile(False)
            for k, v in eng.profile_results().items():
                out.setdefault(k, []).append(v["ms"])
        return {k: statistics.median(v) for k, v in out.items()}

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

    def wall_ms(fn, n=3):
        fn()
        torch.cuda.synchronize()
        tt = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            tt.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(tt)

    rate = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12 if ms > 0 else float("nan")
    trimap = torch.from_numpy(TS.ring(H, W, r=0.33, width=0.03)).cuda()
    image = torch.rand(1, H, W, 3, device="cuda")
    (oy, sy), (ox, sx) = tile_axis(H, args.tile, args.overlap), tile_axis(W, args.tile, args.overlap)
    band_px = int(((trimap > 0.25) & (trimap < 0.75)).sum())

    # ---- band_tiles ----
    call = lambda: eng.band_tiles(trimap, tile=args.tile, overlap=args.overlap, return_count=True)
    tiles, count = call()
    med, lo, hi = median_ms(call)
    per = launches_ms(call, args.runs)
    copy4 = copy_ms(px * 4 // 2)                                      # a copy of n bytes moves 2 n: read and write
    ref = torch_band_tiles(trimap, 0.25, 0.75, oy, sy, ox, sx)
    tiles = compact_boxes(tiles)
    assert [(y0, x0) for _, y0, x0, _, _ in tiles.tolist()] == ref[:16]
    tmed = wall_ms(lambda: torch_band_tiles(trimap, 0.25, 0.75, oy, sy, ox, sx))
    print(f"[tiles_bench] 1x{H}x{W} tile={args.tile} overlap={args.overlap}: {int(count[0])} active tiles of {len(oy)} x {len(ox)} = {len(oy) * len(ox)} grid cells; "
          f"{band_px} band pixels ({100.0 * band_px / px:.2f} %)", flush=True)
    print(f"[tiles_bench] band_tiles: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) | " + " ".join(f"{k} {v:.4f} ms" for k, v in per.items())
          + f" | copy that moves the compulsory 4 B/px {copy4:.4f} ms = {rate(px * 4, copy4):.2f} TB/s | tiles_mark = {per['tiles_mark'] / copy4:.2f} x the copy, "
          f"{rate(px * 4, per['tiles_mark']):.2f} TB/s | torch restatement on the device, median wall {tmed:.2f} ms = {tmed / med:.1f} x the call", flush=True)

    # ---- apply_matte_tiles: tiles_blend from the per-launch profile ----
    copy8 = copy_ms(px * 8 // 2)
    ent = tiles.tolist()
    for S in (int(v) for v in args.S.split(",")):
        call = lambda: eng.apply_matte_tiles(image, trimap, tiles.cuda(), S, False, "alpha_only", False, 0.8, args.feather)
        alpha, _ = call()
        med, lo, hi = median_ms(call)
        per = launches_ms(call, args.runs)
        blend = per["tiles_blend"]
        # the restatement of the blend on what the kernel blends: every slot resized to its tile the way the call does it (apply_matte_node on the crop)
        ic = torch.stack([image[b, y0:y0 + h, x0:x0 + w] for b, y0, x0, h, w in ent]).contiguous()
        tc = torch.stack([trimap[b, y0:y0 + h, x0:x0 + w] for b, y0, x0, h, w in ent]).contiguous()
        crops, _ = eng.apply_matte_node(ic, tc, S, False, "alpha_only", False, 0.8)
        want = torch_blend(crops, ent, trimap, args.feather)
        diff = float((alpha - want).abs().max())
        tmed = wall_ms(lambda: torch_blend(crops, ent, trimap, args.feather))
        print(f"[tiles_bench] apply_matte_tiles N={len(ent)} S={S} feather={args.feather}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) | tiles_blend {blend:.4f} ms | "
              f"boxes_prep_image {per['boxes_prep_image']:.4f} ms boxes_prep_trimap {per['boxes_prep_trimap']:.4f} ms | copy that moves the compulsory 8 B/px "
              f"{copy8:.4f} ms = {rate(px * 8, copy8):.2f} TB/s | tiles_blend = {blend / copy8:.2f} x the copy, {rate(px * 8, blend):.2f} TB/s | torch restatement of "
              f"the blend on the device, median wall {tmed:.2f} ms = {tmed / blend:.1f} x tiles_blend; max |difference| {diff:.2e}", flush=True)
        del ic, tc, crops, want, alpha
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
