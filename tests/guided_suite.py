"""Shared by tests/test_node_guided_cpu.py, tests/test_emu_guided.py and tests/test_gpu_guided.py: the guided-refinement cases, the purpose scene, and a
numpy reference of the function defined in include/sdmatte.h (sdm_refine_alpha_guided) that shares no code with the kernels (csrc/k_guided.h) or with
the torch restatement (sdmatte_nodes.guided_refine_alpha): explicit index arrays, direct window sums, callable in fp64 and in fp32.

Tolerance of `compare`, per case: max(4 * d32, 2**-20) on the max abs difference to reference(fp64).
  * d32 is the larger distance to reference(fp64) of two fp32 evaluations of the reference, one solving the 3 x 3 system with the adjugate, one with
    np.linalg.solve: the sensitivity of the solve to its rounding sequence is inside d32 and not guessed.  It is computed here, never taken from the code
    under test.
  * 4x: another fp32 evaluation differs in summation order, FMA contraction and division sequence, each a perturbation of the size of fp32 rounding;
    the two box stages are means and do not amplify.  (The margin of foreground_suite.py.)
  * floor 2**-20 = 8 ulp of 1.0, for constant inputs.
eps crosses the C ABI as a float, so the reference rounds it to fp32 first: d32 measures arithmetic only."""
import functools

import numpy as np
import torch

import foreground_suite as FS


# ---- reference --------------------------------------------------------------------------------------------------------------------------
def sanitise_alpha(alpha):
    a = np.asarray(alpha, np.float32)
    a = np.where(np.isnan(a), np.float32(0), a)
    return np.minimum(np.maximum(a, np.float32(0)), np.float32(1)).astype(np.float32)


def _block_sum(x, axis, s, n_coarse):
    """Sum of x over blocks [i s, min(N, i s + s)) of `axis`, and the number of existing entries per block."""
    x = np.moveaxis(x, axis, 0)
    N = x.shape[0]
    acc = np.zeros((n_coarse,) + x.shape[1:], x.dtype)
    cnt = np.zeros(n_coarse, np.int64)
    for d in range(s):
        idx = np.arange(n_coarse, dtype=np.int64) * s + d
        ok = idx < N
        acc[ok] += x[idx[ok]]
        cnt += ok
    return np.moveaxis(acc, 0, axis), cnt


def _window_sum(x, axis, radius):
    """Direct sum of x over [i - radius, i + radius] clipped to `axis`, and the number of entries of each window."""
    x = np.moveaxis(x, axis, 0)
    N = x.shape[0]
    acc = np.zeros_like(x)
    cnt = np.zeros(N, np.int64)
    for d in range(-radius, radius + 1):
        idx = np.arange(N, dtype=np.int64) + d
        ok = (idx >= 0) & (idx < N)
        acc[ok] += x[idx[ok]]
        cnt += ok
    return np.moveaxis(acc, 0, axis), cnt


def _upsample_axis(n_full, n_coarse, s, dtype):
    u = np.clip((np.arange(n_full).astype(dtype) + dtype(0.5)) / dtype(s) - dtype(0.5), dtype(0), dtype(n_coarse - 1))
    i0 = np.floor(u).astype(np.int64)
    return i0, np.minimum(i0 + 1, n_coarse - 1), (u - i0.astype(dtype)).astype(dtype)


def reference(image, alpha, subsample, radius, eps, dtype=np.float64, solver="adjugate"):
    """image [B,H,W,3], alpha [B,H,W] -> refined alpha [B,H,W] in `dtype`."""
    s, one, zero = int(subsample), dtype(1), dtype(0)
    eps = dtype(np.float32(eps))
    img = np.asarray(image, np.float32).astype(dtype)
    p = sanitise_alpha(alpha).astype(dtype)
    B, H, W = p.shape
    h, w = -(-H // s), -(-W // s)
    x = np.concatenate([img, p[..., None]], -1)                          # [B,H,W,4]
    x, cy = _block_sum(x, 1, s, h)
    x, cx = _block_sum(x, 2, s, w)
    x = x / (cy[:, None] * cx[None, :]).astype(dtype)[None, :, :, None]
    Ic, pc = x[..., :3], x[..., 3]

    def mean(t):                                                         # t [B,h,w,...]
        t, ny = _window_sum(t, 1, radius)
        t, nx = _window_sum(t, 2, radius)
        n = (ny[:, None] * nx[None, :]).astype(dtype)
        return t / n.reshape((1, h, w) + (1,) * (t.ndim - 3))
    mu, mup = mean(Ic), mean(pc)
    c = mean(Ic * pc[..., None]) - mu * mup[..., None]
    Sig = mean(Ic[..., :, None] * Ic[..., None, :]) - mu[..., :, None] * mu[..., None, :] + eps * np.eye(3, dtype=dtype)
    if solver == "adjugate":
        s00, s01, s02, s11, s12, s22 = Sig[..., 0, 0], Sig[..., 0, 1], Sig[..., 0, 2], Sig[..., 1, 1], Sig[..., 1, 2], Sig[..., 2, 2]
        k00, k01, k02 = s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11
        k11, k12, k22 = s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01
        det = s00 * k00 + s01 * k01 + s02 * k02
        a = np.stack([k00 * c[..., 0] + k01 * c[..., 1] + k02 * c[..., 2], k01 * c[..., 0] + k11 * c[..., 1] + k12 * c[..., 2],
                      k02 * c[..., 0] + k12 * c[..., 1] + k22 * c[..., 2]], -1) / det[..., None]
    else:
        a = np.linalg.solve(Sig, c[..., None])[..., 0]
    b = mup - (a * mu).sum(-1)
    assert a.dtype == dtype and b.dtype == dtype
    ab = mean(np.concatenate([a, b[..., None]], -1))                     # [B,h,w,4]
    i0, i1, fy = _upsample_axis(H, h, s, dtype)
    j0, j1, fx = _upsample_axis(W, w, s, dtype)
    rows = (one - fy)[None, :, None, None] * ab[:, i0] + fy[None, :, None, None] * ab[:, i1]                 # [B,H,w,4]
    up = (one - fx)[None, None, :, None] * rows[:, :, j0] + fx[None, None, :, None] * rows[:, :, j1]         # [B,H,W,4]
    out = np.minimum(np.maximum((up[..., :3] * img).sum(-1) + up[..., 3], zero), one)
    assert out.dtype == dtype
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 300), (130, 1), (33, 70), (97, 131), (150, 200)]
TRIPLES = [(1, 4, 1e-4), (2, 3, 1e-3), (4, 2, 1e-4), (7, 1, 1e-4), (16, 1, 1e-4), (1, 32, 1e-6), (3, 32, 1e-4)]      # (subsample, radius, eps)
PATTERNS = ["soft", "hard", "const0", "const1", "noise", "dirty"]


def _inputs(pattern, seed, B, H, W):
    image, alpha, _, _ = FS.scene(seed, B, H, W)
    rng = np.random.default_rng(seed + 2000)
    # the noise keeps Sigma non-degenerate away from the edge
    image = np.clip(image + rng.normal(0.0, 0.02, image.shape), 0.0, 1.0).astype(np.float32)
    if pattern == "hard":
        alpha = (alpha > 0.5).astype(np.float32)
    elif pattern.startswith("const"):
        alpha = np.full_like(alpha, {"const0": 0.0, "const1": 1.0}[pattern])
    elif pattern == "noise":
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
    """((name, image, alpha, (subsample, radius, eps)), ...) at B = 2: every size with every triple (42 cases), the alpha patterns in turn."""
    out = []
    for i, (H, W) in enumerate(SIZES):
        for j, (s, r, eps) in enumerate(TRIPLES):
            pat = PATTERNS[(i + j) % len(PATTERNS)]
            out.append((f"{pat}_{H}x{W}_s{s}_r{r}_eps{eps:g}", *_inputs(pat, 10 * i + j, 2, H, W), (s, r, eps)))
    return tuple(out)


def references_for(image, alpha, params):
    """(reference in fp64, d32)"""
    r64 = reference(image, alpha, *params, dtype=np.float64)
    d32 = max(float(np.abs(reference(image, alpha, *params, dtype=np.float32, solver=sv) - r64).max()) for sv in ("adjugate", "solve"))
    return r64, d32


@functools.lru_cache(maxsize=None)
def _references(name):
    """Computed once per process and shared by every test that needs it."""
    _, image, alpha, params = next(c for c in cases() if c[0] == name)
    return references_for(image, alpha, params)


def tolerance(d32):
    return max(4.0 * d32, 2.0 ** -20)


def compare(name, out, refs, report=None):
    """out (a torch tensor on any device) against the references of a case, under the rule above."""
    r64, d32 = refs
    tol = tolerance(d32)
    out = out.detach().cpu()
    assert out.dtype == torch.float32 and tuple(out.shape) == r64.shape, (name, out.dtype, tuple(out.shape))
    out = out.numpy()
    assert np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0, name
    d = float(np.abs(out.astype(np.float64) - r64).max())
    line = f"[guided] {name}: d32 = {d32:.3e} tol = {tol:.3e} d = {d:.3e} ratio = {d / max(d32, 1e-30):.2f}"
    print(line)
    if report is not None:
        report.append(line)
    assert d <= tol, line


def check(refine, to_tensor, report=None):
    """refine(image, alpha, subsample, radius, eps) -> alpha on tensors made by `to_tensor` from CPU tensors; every case."""
    for name, image, alpha, params in cases():
        out = refine(to_tensor(torch.from_numpy(image)), to_tensor(torch.from_numpy(alpha)), *params)
        compare(name, out, _references(name), report)


# ---- what the call is for ---------------------------------------------------------------------------------------------------------------
PURPOSE = (4, 2, 1e-4)          # (subsample, radius, eps)


@functools.lru_cache(maxsize=None)
def purpose_scene():
    """(image [1,256,384,3], true alpha, bilinear alpha): a composite with a 2-pixel edge, and its alpha after an antialiased bilinear reduction by 4
    and a bilinear enlargement back - what a model that saw a quarter of the resolution returns."""
    import torch.nn.functional as F
    _, alpha, Fg, Bg = FS.scene(5, 1, 256, 384)
    alpha = np.clip(0.5 + (alpha.astype(np.float64) - 0.5) * max(2.0, 0.12 * 256) / 2.0, 0.0, 1.0)
    image = (alpha[..., None] * Fg + (1.0 - alpha[..., None]) * Bg).astype(np.float32)
    alpha = alpha.astype(np.float32)
    small = F.interpolate(torch.from_numpy(alpha)[:, None], size=(64, 96), mode="bilinear", antialias=True, align_corners=False)
    blurred = F.interpolate(small, size=(256, 384), mode="bilinear", align_corners=False)[:, 0].clamp(0.0, 1.0).numpy()
    return image, alpha, blurred


def check_purpose(refined, what):
    """max |refined - true| <= 0.5 max |bilinear - true| and the mean no larger than the bilinear alpha's."""
    _, true, blurred = purpose_scene()
    refined = np.asarray(refined, np.float64).reshape(true.shape)
    e_ref, e_bil = np.abs(refined - true), np.abs(blurred.astype(np.float64) - true)
    line = f"[guided] purpose ({what}): max {e_bil.max():.4f} -> {e_ref.max():.4f}, mean {e_bil.mean():.3e} -> {e_ref.mean():.3e}"
    print(line)
    assert e_ref.max() <= 0.5 * e_bil.max() and e_ref.mean() <= e_bil.mean(), line
    return line
