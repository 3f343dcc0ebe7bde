"""Shared by tests/test_node_foreground_cpu.py, tests/test_emu_foreground.py and tests/test_gpu_foreground.py: the foreground-estimation cases, a
synthetic composite with known foreground, and a numpy reference of the function defined in include/sdmatte.h (sdm_estimate_foreground) that shares
no code with the kernels (csrc/k_foreground.h) or with the torch restatement (sdmatte_nodes.estimate_foreground): explicit index arrays, callable
in fp64 and in fp32.

Tolerance of `check`, per case: max(4 * d32, 2**-20) on the max abs difference of fg and of bg to reference(fp64), where d32 is the largest
distance of reference(fp32) to reference(fp64) for that case - computed here, never taken from the code under test.
  * 4x: a step is a non-expansive weighted mean plus a bounded correction, so rounding differences add over the 60 - 70 steps and do not grow; another
    fp32 evaluation differs from fp32 numpy in FMA contraction, summation order and its division sequence, each a perturbation of the size of fp32
    rounding itself.
  * floor 2**-20 = 8 ulp of 1.0, for cases where d32 happens to be about 1e-9 (constant alpha).
The parameters cross the C ABI as floats, so the reference rounds them to fp32 first: d32 measures arithmetic only."""
import functools

import numpy as np
import torch

DEFAULTS = {"regularization": 1e-5, "gradient_weight": 1.0, "n_small_iters": 10, "n_big_iters": 2}
SMALL = 32


# ---- reference --------------------------------------------------------------------------------------------------------------------------
def level_sizes(H, W):
    """[(H, W), (ceil(H/2), ceil(W/2)), ..., (1, 1)]"""
    out = [(H, W)]
    while out[-1] != (1, 1):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def n_large_levels(H, W):
    return sum(1 for h, w in level_sizes(H, W) if max(h, w) > SMALL)


def sanitise_alpha(alpha):
    a = np.asarray(alpha, np.float32)
    a = np.where(np.isnan(a), np.float32(0), a)
    return np.minimum(np.maximum(a, np.float32(0)), np.float32(1)).astype(np.float32)


def _src(nd, ns):
    return np.minimum(ns - 1, (np.arange(nd, dtype=np.int64) * ns) // nd)


def reference(image, alpha, params=None, dtype=np.float64):
    """image [B,H,W,3], alpha [B,H,W] -> (fg [B,H,W,3], bg [B,H,W,3]) in `dtype`."""
    p = dict(DEFAULTS, **(params or {}))
    reg, gw = dtype(np.float32(p["regularization"])), dtype(np.float32(p["gradient_weight"]))
    img = np.asarray(image, np.float32).astype(dtype)
    alp = sanitise_alpha(alpha).astype(dtype)
    H, W = img.shape[1:3]
    one, zero = dtype(1), dtype(0)
    F = Bc = None
    for h, w in reversed(level_sizes(H, W)):
        ys, xs = _src(h, H)[:, None], _src(w, W)[None, :]
        I = img[:, ys, xs, :]
        a0 = alp[:, ys, xs][..., None]
        if F is None:
            F, Bc = I.copy(), I.copy()
        else:
            py, px = _src(h, F.shape[1])[:, None], _src(w, F.shape[2])[None, :]
            F, Bc = F[:, py, px, :], Bc[:, py, px, :]
        yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
        nbr = ((yy, np.maximum(xx - 1, 0)), (yy, np.minimum(xx + 1, w - 1)), (np.maximum(yy - 1, 0), xx), (np.minimum(yy + 1, h - 1), xx))
        a1 = one - a0
        wq = [reg + gw * np.abs(a0 - a0[:, qy, qx]) for qy, qx in nbr]
        s = wq[0] + wq[1] + wq[2] + wq[3]
        D = a0 * a0 + a1 * a1 + s
        for _ in range(p["n_small_iters"] if max(h, w) <= SMALL else p["n_big_iters"]):
            Fm = (wq[0] * F[:, nbr[0][0], nbr[0][1]] + wq[1] * F[:, nbr[1][0], nbr[1][1]] + wq[2] * F[:, nbr[2][0], nbr[2][1]]
                  + wq[3] * F[:, nbr[3][0], nbr[3][1]]) / s
            Bm = (wq[0] * Bc[:, nbr[0][0], nbr[0][1]] + wq[1] * Bc[:, nbr[1][0], nbr[1][1]] + wq[2] * Bc[:, nbr[2][0], nbr[2][1]]
                  + wq[3] * Bc[:, nbr[3][0], nbr[3][1]]) / s
            r = (I - a0 * Fm - a1 * Bm) / D
            F = np.minimum(np.maximum(Fm + a0 * r, zero), one)
            Bc = np.minimum(np.maximum(Bm + a1 * r, zero), one)
        assert F.dtype == dtype and Bc.dtype == dtype
    return F, Bc


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def scene(seed, B, H, W):
    """A smooth synthetic composite: (image, alpha, F, Bg) as fp32 arrays.  Per image and channel F and Bg are low-frequency ramps (F in about
    [0.5, 1], Bg in about [0, 0.4]); alpha is a disk of radius 0.3 min(H, W) with a linear edge of width max(2, 0.12 min(H, W)) whose centre is
    random inside the middle 40 % and differs per image; image = alpha F + (1 - alpha) Bg."""
    rng = np.random.default_rng(seed)
    v = (np.arange(H, dtype=np.float64) / max(H - 1, 1) * 2 - 1)[None, :, None, None]
    u = (np.arange(W, dtype=np.float64) / max(W - 1, 1) * 2 - 1)[None, None, :, None]

    def ramp(lo, hi, amp=0.1):
        # a base colour per image and channel plus a plane of at most +- amp across the image.  The estimator continues F into the pixels where
        # alpha is small from where alpha is large, so its error there is about (slope of F) x (edge width): the ramps are gentle (0.2 across the
        # whole image), the base colours carry the contrast between F and Bg
        c = rng.uniform(-1, 1, (2, B, 1, 1, 3))
        c = c / np.maximum(np.abs(c).sum(0, keepdims=True), 1.0)           # |cu| + |cv| <= 1: the plane stays within +- amp
        return rng.uniform(lo + amp, hi - amp, (B, 1, 1, 3)) + amp * (c[0] * u + c[1] * v)
    F, Bg = ramp(0.5, 1.0), ramp(0.0, 0.4)
    m = min(H, W)
    cy = (0.3 + 0.4 * rng.uniform(size=(B, 1, 1))) * H
    cx = (0.3 + 0.4 * rng.uniform(size=(B, 1, 1))) * W
    d = np.sqrt((np.arange(H)[None, :, None] + 0.5 - cy) ** 2 + (np.arange(W)[None, None, :] + 0.5 - cx) ** 2)
    alpha = np.clip(0.5 + (0.3 * m - d) / max(2.0, 0.12 * m), 0.0, 1.0)
    image = alpha[..., None] * F + (1 - alpha[..., None]) * Bg
    return image.astype(np.float32), alpha.astype(np.float32), F.astype(np.float32), Bg.astype(np.float32)


SIZES = [(97, 131), (5, 300), (1, 1), (1, 300), (130, 1), (32, 32), (33, 70), (150, 200)]
PATTERNS = ["soft", "hard", "const0", "const05", "const1", "noise", "dirty"]
VARIANTS = [("reg1e-3_gw0", {"regularization": 1e-3, "gradient_weight": 0.0}), ("iters3_1", {"n_small_iters": 3, "n_big_iters": 1}),
            ("big4", {"n_big_iters": 4})]


def _inputs(pattern, seed, B, H, W):
    image, alpha, _, _ = scene(seed, B, H, W)
    rng = np.random.default_rng(seed + 1000)
    if pattern == "hard":
        alpha = (alpha > 0.5).astype(np.float32)
    elif pattern.startswith("const"):
        alpha = np.full_like(alpha, {"const0": 0.0, "const05": 0.5, "const1": 1.0}[pattern])
    elif pattern == "noise":          # every pixel, tile seam and border moves in every step
        alpha = rng.uniform(size=alpha.shape).astype(np.float32)
        image = rng.uniform(size=image.shape).astype(np.float32)
    elif pattern == "dirty":          # soft, with NaN and values outside [0, 1] sprinkled in
        alpha = alpha.copy()
        pick = rng.uniform(size=alpha.shape)
        alpha[pick < 0.03] = np.nan
        alpha[(pick >= 0.03) & (pick < 0.06)] = -0.5
        alpha[(pick >= 0.06) & (pick < 0.09)] = 1.5
    return image, alpha


@functools.lru_cache(maxsize=None)
def cases():
    """((name, image, alpha, params), ...): every size at B = 2 crossed with the alpha patterns, and the parameter variants at two sizes."""
    out = []
    for i, (H, W) in enumerate(SIZES):
        for j, pat in enumerate(PATTERNS):
            out.append((f"{pat}_{H}x{W}", *_inputs(pat, 10 * i + j, 2, H, W), {}))
    for H, W in ((97, 131), (150, 200)):
        for name, params in VARIANTS:
            out.append((f"soft_{name}_{H}x{W}", *_inputs("soft", H, 2, H, W), dict(params)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _references(name):
    """(fg64, bg64, d32) of a case, computed once per process and shared by every test that needs it."""
    _, image, alpha, params = next(c for c in cases() if c[0] == name)
    return references_for(image, alpha, params)


def references_for(image, alpha, params):
    f64, b64 = reference(image, alpha, params, np.float64)
    f32, b32 = reference(image, alpha, params, np.float32)
    d32 = max(float(np.abs(f32 - f64).max()), float(np.abs(b32 - b64).max()))
    return f64, b64, d32


def tolerance(d32):
    return max(4.0 * d32, 2.0 ** -20)


def compare(name, fg, bg, alpha, refs, rgba, report=None):
    """fg / bg (torch tensors, any device; bg may be None) against the references of a case, under the rule above."""
    f64, b64, d32 = refs
    tol = tolerance(d32)
    fg = fg.detach().cpu()
    assert fg.dtype == torch.float32 and tuple(fg.shape) == f64.shape[:3] + (4 if rgba else 3,), (name, fg.dtype, tuple(fg.shape))
    fg = fg.numpy()
    assert np.isfinite(fg).all() and fg.min() >= 0.0 and fg.max() <= 1.0, name
    if rgba:
        assert np.array_equal(fg[..., 3], sanitise_alpha(alpha)), name
    d_fg = float(np.abs(fg[..., :3].astype(np.float64) - f64).max())
    d_bg = 0.0
    if bg is not None:
        bg = bg.detach().cpu()
        assert bg.dtype == torch.float32 and tuple(bg.shape) == b64.shape, (name, bg.dtype, tuple(bg.shape))
        bg = bg.numpy()
        assert np.isfinite(bg).all() and bg.min() >= 0.0 and bg.max() <= 1.0, name
        d_bg = float(np.abs(bg.astype(np.float64) - b64).max())
    line = f"[foreground] {name}: d32 = {d32:.3e} tol = {tol:.3e} d_fg = {d_fg:.3e} d_bg = {d_bg:.3e} ratio = {max(d_fg, d_bg) / max(d32, 1e-30):.2f}"
    print(line)
    if report is not None:
        report.append(line)
    assert d_fg <= tol and d_bg <= tol, line


def check(estimate, to_tensor, report=None):
    """estimate(image, alpha, params, rgba) -> (fg, bg) on tensors made by `to_tensor` from CPU tensors; every case, alternating fg_channels 3 / 4."""
    for i, (name, image, alpha, params) in enumerate(cases()):
        rgba = i % 2 == 1
        fg, bg = estimate(to_tensor(torch.from_numpy(image)), to_tensor(torch.from_numpy(alpha)), params, rgba)
        compare(name, fg, bg, alpha, _references(name), rgba, report)
