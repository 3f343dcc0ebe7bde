"""Shared by tests/test_emu_trimap.py, tests/test_node_trimap_cpu.py and tests/test_gpu_trimap.py: the trimap-from-mask cases and two references
that share no code with the kernels (csrc/k_trimap.h) or with the CPU restatement (sdmatte_nodes.trimap_from_mask):
  * `brute_force`: for every integer offset of the closed disk, shift and OR - the definition itself;
  * `separable`:  a column sweep with running counters, then a windowed row pass - for sizes where the brute force takes too long; proven equal
                  to the brute force on every small case by tests/test_node_trimap_cpu.py.
Every comparison is exact (np.array_equal / torch.equal): the trimap is made of compares and integer arithmetic only."""
import math

import numpy as np
import torch


# ---- references -------------------------------------------------------------------------------------------------------------------------
def _foreground(mask, threshold):
    with np.errstate(invalid="ignore"):
        return np.asarray(mask, np.float32) > np.float32(threshold)      # one fp32 compare: NaN is background


def _or_over_disk(src, r):
    """out[p] = OR of src[p + o] over the integer offsets o of the closed disk of radius r; pixels beyond the border do not exist."""
    _, H, W = src.shape
    out = np.zeros_like(src)
    for dy in range(-min(r, H - 1), min(r, H - 1) + 1):
        for dx in range(-min(r, W - 1), min(r, W - 1) + 1):
            if dx * dx + dy * dy > r * r:
                continue
            y0, y1, x0, x1 = max(0, -dy), H - max(0, dy), max(0, -dx), W - max(0, dx)
            out[:, y0:y1, x0:x1] |= src[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def _compose(fg, near_bg, near_fg):
    out = fg.astype(np.float32)
    out[(fg & near_bg) | (~fg & near_fg)] = 0.5
    return out


def brute_force(mask, threshold, erode_px, dilate_px):
    fg = _foreground(mask, threshold)
    return _compose(fg, _or_over_disk(~fg, erode_px), _or_over_disk(fg, dilate_px))


def _column_sweep(src):
    """Vertical distance to the nearest True in the column (0 on a True pixel), by running counters down and up."""
    _, H, _ = src.shape
    far = 1 << 20
    d = np.full(src.shape, far, np.int64)
    run = np.full(src[:, 0].shape, far, np.int64)
    for y in range(H):
        run = np.where(src[:, y], 0, run + 1)
        d[:, y] = run
    run = np.full(src[:, 0].shape, far, np.int64)
    for y in range(H - 1, -1, -1):
        run = np.where(src[:, y], 0, run + 1)
        d[:, y] = np.minimum(d[:, y], run)
    return d


def _or_over_disk_separable(src, r):
    _, _, W = src.shape
    d = _column_sweep(src)
    out = np.zeros_like(src)
    for dx in range(-min(r, W - 1), min(r, W - 1) + 1):
        h = math.isqrt(r * r - dx * dx)
        x0, x1 = max(0, -dx), W - max(0, dx)
        out[:, :, x0:x1] |= d[:, :, x0 + dx:x1 + dx] <= h
    return out


def separable(mask, threshold, erode_px, dilate_px):
    fg = _foreground(mask, threshold)
    return _compose(fg, _or_over_disk_separable(~fg, erode_px), _or_over_disk_separable(fg, dilate_px))


# ---- masks ------------------------------------------------------------------------------------------------------------------------------
def blobs(seed, B, H, W, n=6):
    """Soft random blobs in [0, 1]: a few Gaussian bumps per image (different per image)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.zeros((B, H, W), np.float32)
    for b in range(B):
        for _ in range(n):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            s = rng.uniform(0.04, 0.2) * max(H, W)
            out[b] = np.maximum(out[b], np.exp(-((ys - cy) ** 2 + (xs - cx) ** 2) / (2 * s * s)).astype(np.float32))
    return out


SIZES = [(97, 131), (5, 300)]      # neither a multiple of a kernel tile (64 columns, 256-pixel row segments); the second is shorter than most radii


def small_cases():
    """[(name, mask fp32 [2,H,W], threshold, erode_px, dilate_px)] - every case of the issue's list, at both sizes."""
    out = []
    for H, W in SIZES:
        tag = f"{H}x{W}"
        bl = blobs(H * 1000 + W, 2, H, W)
        out.append((f"blobs_{tag}", bl, 0.5, 4, 4))
        out.append((f"blobs_erode_ne_dilate_{tag}", bl, 0.35, 3, 9))
        out.append((f"blobs_dilate_only_{tag}", bl, 0.5, 0, 6))
        out.append((f"blobs_erode_only_{tag}", bl, 0.5, 6, 0))
        out.append((f"radius_zero_{tag}", bl, 0.5, 0, 0))
        out.append((f"radius_larger_than_image_{tag}", bl, 0.6, min(255, max(H, W) + 9), min(255, max(H, W) + 30)))
        out.append((f"radius_between_h_and_w_{tag}", bl, 0.6, 70, 17))
        lines = np.zeros((2, H, W), np.float32)
        lines[0, H // 2, :] = 1.0                                           # 1 px, horizontal, touching both borders
        lines[0, :, W // 3:W // 3 + 2] = 1.0                                # 2 px, vertical
        for i in range(min(H, W)):                                          # 1 px diagonal
            lines[1, i, i] = 1.0
        lines[1, : max(1, H // 2), W - 7] = 1.0
        out.append((f"thin_lines_{tag}", lines, 0.5, 1, 5))
        out.append((f"thin_lines_inverted_{tag}", 1.0 - lines, 0.5, 5, 2))
        dots = np.zeros((2, H, W), np.float32)
        rng = np.random.default_rng(7)
        for b in range(2):
            for _ in range(5):
                dots[b, rng.integers(0, H), rng.integers(0, W)] = 1.0
        dots[0, 0, 0] = dots[0, H - 1, W - 1] = 1.0
        out.append((f"isolated_pixels_{tag}", dots, 0.5, 2, 6))
        out.append((f"isolated_holes_{tag}", 1.0 - dots, 0.5, 6, 2))
        border = np.zeros((2, H, W), np.float32)
        border[0, : max(1, H // 3), W // 4: W // 2] = 1.0                   # top
        border[0, H - max(1, H // 4):, W // 2 + 9:] = 1.0                   # bottom + right (corner)
        border[1, :, : W // 5] = 1.0                                        # left, full height
        border[1, H // 3: H // 3 + 2, W - 20:] = 1.0                        # right
        out.append((f"touching_borders_{tag}", border, 0.5, 5, 8))
        out.append((f"all_foreground_{tag}", np.ones((2, H, W), np.float32), 0.5, 7, 7))
        out.append((f"all_background_{tag}", np.zeros((2, H, W), np.float32), 0.5, 7, 7))
        odd = bl.copy()
        odd[0, ::3, ::5] = np.nan                                           # NaN: background
        odd[1, :, : W // 2] = np.float32(0.3)                               # exactly the threshold: background (strict >)
        odd[1, H // 2, W // 4] = np.nextafter(np.float32(0.3), np.float32(1.0))
        out.append((f"nan_and_equal_to_threshold_{tag}", odd, 0.3, 2, 3))
    return out


def check_make_trimap(make, to_tensor, cases=None):
    """make(mask tensor, threshold, erode_px, dilate_px) -> trimap tensor; every case equals the brute force, bit for bit."""
    for name, mask, thr, e, d in (cases if cases is not None else small_cases()):
        got = make(to_tensor(torch.from_numpy(mask)), thr, e, d).cpu().numpy()
        want = brute_force(mask, thr, e, d)
        assert got.dtype == np.float32 and got.shape == want.shape, name
        assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} of {want.size} pixels differ"
        assert set(np.unique(got).tolist()) <= {0.0, 0.5, 1.0}, name


# ---- apply_matte_mask == make_trimap + apply_matte_node ---------------------------------------------------------------------------------
def e2e_inputs(B=1, H=50, W=70, seed=5):
    """Image and soft mask NOT at the inference size (64): the node resizes both."""
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(B, H, W, 3, generator=g)
    mask = torch.from_numpy(blobs(seed, B, H, W, n=3))
    return image, mask


def check_mask_call_equals_two_calls(eng, to_tensor, modes=("alpha_only", "matted_rgba", "matted_rgb"), refines=(False, True), S=64, B=1):
    """Engine.apply_matte_mask is bit-identical, in alpha, matted and trimap, to make_trimap followed by apply_matte_node; each call launches the two
    trimap kernels once; a mask of another size than the image passes where nothing indexes the alpha with the trimap, and raises where something does."""
    image, mask = e2e_inputs(B)
    image, mask = to_tensor(image), to_tensor(mask)
    thr, e, d = 0.4, 3, 5
    for mode in modes:
        for refine in refines:
            eng.lib.kernel_counts(reset=True)
            a, m, t = eng.apply_matte_mask(image, mask, S, False, mode, refine, 0.8, thr, e, d)      # (an SDM_ERR_ARENA would raise here)
            counts = eng.lib.kernel_counts()
            assert counts.get("trimap_cols") == 1 and counts.get("trimap_rows") == 1, counts
            t2 = eng.make_trimap(mask, thr, e, d)
            a2, m2 = eng.apply_matte_node(image, t2, S, False, mode, refine, 0.8)
            assert torch.equal(t, t2) and torch.equal(a, a2) and torch.equal(m, m2), (mode, refine)
            assert np.array_equal(t.cpu().numpy(), brute_force(mask.cpu().numpy(), thr, e, d))
    small = to_tensor(torch.from_numpy(blobs(9, B, 29, 41, n=3)))
    a, m, t = eng.apply_matte_mask(image, small, S, False, "matted_rgba", False, 0.8, thr, e, d)
    t2 = eng.make_trimap(small, thr, e, d)
    a2, m2 = eng.apply_matte_node(image, t2, S, False, "matted_rgba", False, 0.8)
    assert t.shape == small.shape and torch.equal(t, t2) and torch.equal(a, a2) and torch.equal(m, m2)
    for mode, refine in (("alpha_only", True), ("matted_rgb", False)):
        try:
            eng.apply_matte_mask(image, small, S, False, mode, refine, 0.8, thr, e, d)
        except IndexError:
            continue
        raise AssertionError(f"a mask of another size must raise the size error for {mode}, mask_refine={refine}")
