"""Shared by tests/test_node_temporal_cpu.py, tests/test_emu_temporal.py and tests/test_gpu_temporal.py: the temporal-smoothing cases, the purpose scene,
and a numpy reference of the function defined in include/sdmatte.h (sdm_smooth_alpha_temporal) that shares no code with the kernel (csrc/k_temporal.h)
or with the torch restatement (sdmatte_nodes.temporal_smooth_alpha): explicit index loops over k and over the patch offsets, callable in fp64 and fp32.

Tolerance of `compare`, per case: max(4 * d32, 2**-20) on the max abs difference to reference(fp64).
  * d32 is the larger distance to reference(fp64) of two fp32 evaluations of the reference that differ in summation order: one sums the patch row-major
    and takes k ascending, the other sums it separably (along x, then along y) and takes k descending.  It is computed here, never taken from the code
    under test.
  * 4x: another fp32 evaluation differs in summation order, FMA contraction and division sequence, each a perturbation of the size of fp32 rounding; the
    function is continuous in every input (the weight is a clamped polynomial of D, the filter a mean whose denominator is at least 1), so nothing
    amplifies.  (The margin of guided_suite.py and foreground_suite.py.)
  * floor 2**-20 = 8 ulp of 1.0, for constant inputs.
color_tolerance, strength and max_change cross the C ABI as floats and tau2 is one fp32 product, so the reference rounds them the same way first: d32
measures arithmetic only."""
import functools

import numpy as np
import torch


# ---- reference --------------------------------------------------------------------------------------------------------------------------
def sanitise_alpha(alpha):
    a = np.asarray(alpha, np.float32)
    a = np.where(np.isnan(a), np.float32(0), a)
    return np.minimum(np.maximum(a, np.float32(0)), np.float32(1)).astype(np.float32)


def _shift_add(acc, src, dy, dx):
    """acc[y, x] += src[y + dy, x + dx] wherever the source pixel exists"""
    H, W = acc.shape
    ya, yb, xa, xb = max(0, -dy), H - max(0, dy), max(0, -dx), W - max(0, dx)
    if ya < yb and xa < xb:
        acc[ya:yb, xa:xb] += src[ya + dy:yb + dy, xa + dx:xb + dx]


def _patch_sum(e, patch, separable):
    if not separable:
        acc = np.zeros_like(e)
        for dy in range(-patch, patch + 1):
            for dx in range(-patch, patch + 1):
                _shift_add(acc, e, dy, dx)
        return acc
    rows = np.zeros_like(e)
    for dx in range(-patch, patch + 1):
        _shift_add(rows, e, 0, dx)
    acc = np.zeros_like(e)
    for dy in range(-patch, patch + 1):
        _shift_add(acc, rows, dy, 0)
    return acc


def reference(image, alpha, radius, patch, color_tolerance, strength, max_change, clip_len, dtype=np.float64, variant=0):
    """image [B,H,W,3], alpha [B,H,W] -> smoothed alpha [B,H,W] in `dtype`.  variant 0: row-major patch sums, k ascending; 1: separable, k descending."""
    one, zero = dtype(1), dtype(0)
    t32 = np.float32(color_tolerance)
    tau2, strength, max_change = dtype(np.float32(t32 * t32)), dtype(np.float32(strength)), dtype(np.float32(max_change))
    img = np.asarray(image, np.float32).astype(dtype)
    a = sanitise_alpha(alpha).astype(dtype)
    B, H, W = a.shape
    L = int(clip_len) if clip_len else B
    n3 = dtype(3) * _patch_sum(np.ones((H, W), dtype), patch, False)
    out = np.empty_like(a)
    ks = [k for k in range(-radius, radius + 1) if k != 0]
    if variant:
        ks = ks[::-1]
    for t in range(B):
        num, den = a[t].copy(), np.ones((H, W), dtype)
        for k in ks:
            s = t + k
            if s < 0 or s >= B or s // L != t // L:
                continue
            d = img[s] - img[t]
            e = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            D = _patch_sum(e, patch, bool(variant)) / n3
            u = one - D / tau2
            u = np.where(u > zero, u, zero)
            w = strength * (one - dtype(abs(k)) / dtype(radius + 1)) * (u * u)
            num = num + w * a[s]
            den = den + w
        f = num / den
        out[t] = np.minimum(np.maximum(a[t] + np.minimum(np.maximum(f - a[t], -max_change), max_change), zero), one)
    assert out.dtype == dtype
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
DEFAULTS = {"radius": 2, "patch": 1, "color_tolerance": 0.1, "strength": 1.0, "max_change": 1.0, "clip_len": 0}
PATTERNS = ["moving", "static", "cut", "noise", "const0", "const1", "dirty"]


def _lowfreq(rng, H, W, cell=16):
    """A smooth random field of about unit variance: normal values on a grid of `cell` pixels, interpolated bilinearly."""
    gh, gw = H // cell + 2, W // cell + 2
    g = rng.normal(size=(gh, gw))
    y, x = np.arange(H) / cell, np.arange(W) / cell
    i, j = y.astype(int), x.astype(int)
    fy, fx = (y - i)[:, None], (x - j)[None, :]
    return ((1 - fy) * (1 - fx) * g[i][:, j] + (1 - fy) * fx * g[i][:, j + 1] + fy * (1 - fx) * g[i + 1][:, j] + fy * fx * g[i + 1][:, j + 1])


def _background(H, W, phase):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([0.35 + 0.15 * np.sin(x / 9.0 + phase) * np.cos(y / 11.0), 0.45 + 0.15 * np.sin(y / 7.0 + 1.0 + phase),
                     0.30 + 0.10 * np.cos((x + y) / 13.0 + phase)], -1)


def moving_disk(seed, B, H, W, speed=3.0, noise=0.01, jitter=0.08):
    """(image [B,H,W,3], true alpha, observed alpha): a soft disk of a clearly different colour moving `speed` pixels per frame over a static, smoothly
    textured background, per-frame Gaussian colour noise, and the true alpha plus `jitter` times a per-frame low-frequency random field."""
    rng = np.random.default_rng(seed)
    bg = _background(H, W, 0.0)
    fg = np.array([0.9, 0.15, 0.1])
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    r = 0.28 * min(H, W)
    image, true, obs = [], [], []
    for t in range(B):
        cy, cx = 0.5 * H, 0.5 * W - 0.5 * speed * (B - 1) + speed * t
        d = np.sqrt((y - cy) ** 2 + (x - cx) ** 2) - r
        al = np.clip(0.5 - d / 2.0, 0.0, 1.0)
        image.append(al[..., None] * fg + (1.0 - al[..., None]) * bg + rng.normal(0.0, noise, (H, W, 3)))
        true.append(al)
        obs.append(np.clip(al + jitter * _lowfreq(rng, H, W), 0.0, 1.0))
    return np.stack(image).astype(np.float32), np.stack(true).astype(np.float32), np.stack(obs).astype(np.float32)


def cut_scene(seed, B1, B2, H, W):
    """(image, alpha) of B1 + B2 frames with a hard cut between them: the first shot's colours lie in [0, 0.3], the second's in [0.7, 1], so every
    channel differs by at least 0.4 across the cut and every D there is at least 0.16 (>= tau2 for color_tolerance <= 0.4)."""
    rng = np.random.default_rng(seed)
    im1, _, a1 = moving_disk(seed + 1, B1, H, W)
    im2, _, a2 = moving_disk(seed + 2, B2, H, W, speed=-2.0)
    image = np.concatenate([0.3 * np.clip(im1, 0.0, 1.0), 0.7 + 0.3 * np.clip(im2, 0.0, 1.0)]).astype(np.float32)
    assert float(np.abs(image[:B1].max() - image[B1:].min())) >= 0.4
    alpha = np.concatenate([a1, a2]) + rng.normal(0.0, 0.02, (B1 + B2, H, W))
    return image, np.clip(alpha, 0.0, 1.0).astype(np.float32)


def _inputs(pattern, seed, B, H, W):
    rng = np.random.default_rng(seed + 3000)
    image, _, alpha = moving_disk(seed, B, H, W)
    if pattern == "static":            # the picture does not change at all: only the alpha shimmers
        image = np.repeat(image[:1], B, 0)
    elif pattern == "cut" and B >= 2:
        image, alpha = cut_scene(seed, B // 2, B - B // 2, H, W)
    elif pattern == "noise":
        image = rng.uniform(size=image.shape).astype(np.float32)
        alpha = rng.uniform(size=alpha.shape).astype(np.float32)
    elif pattern.startswith("const"):
        alpha = np.full_like(alpha, {"const0": 0.0, "const1": 1.0}[pattern])
    elif pattern == "dirty":           # NaN and values outside [0, 1] sprinkled in
        alpha = alpha.copy()
        pick = rng.uniform(size=alpha.shape)
        alpha[pick < 0.03] = np.nan
        alpha[(pick >= 0.03) & (pick < 0.06)] = -0.5
        alpha[(pick >= 0.06) & (pick < 0.09)] = 1.5
    return np.ascontiguousarray(image), np.ascontiguousarray(alpha)


def _case_specs():
    specs = []                                                             # (B, H, W, overrides)
    for radius in (1, 2, 4):                                               # ring start, wrap, wrapping twice
        for B in sorted({1, 2, radius, radius + 1, 2 * radius + 1, 2 * radius + 2, 11}):
            specs.append((B, 33, 70, {"radius": radius}))
    for i, (H, W) in enumerate([(1, 1), (1, 70), (37, 1), (9, 130), (33, 72), (9, 132)]):      # (W % 4 == 0: the 16-byte load path)
        specs.append((5, H, W, {"patch": i % 3}))
    specs += [(6, 33, 70, {"patch": 0}), (6, 33, 70, {"patch": 2}), (7, 37, 72, {"radius": 4, "patch": 2}), (4, 37, 1, {"radius": 1, "patch": 2})]
    specs += [(8, 20, 40, {"clip_len": c}) for c in (0, 1, 3)]             # 3: a ragged last clip
    specs += [(6, 33, 70, {"strength": 0.5}), (6, 33, 70, {"max_change": 0.05}), (6, 33, 70, {"strength": 0.5, "max_change": 0.05, "radius": 1})]
    specs += [(6, 20, 70, {"color_tolerance": c}) for c in (1.0 / 1024.0, 0.02, 1.0)]
    return specs


def params_of(overrides):
    p = dict(DEFAULTS, **overrides)
    return tuple(p[k] for k in ("radius", "patch", "color_tolerance", "strength", "max_change", "clip_len"))


@functools.lru_cache(maxsize=None)
def cases():
    """((name, image, alpha, (radius, patch, color_tolerance, strength, max_change, clip_len)), ...), the content patterns in turn."""
    out = []
    for i, (B, H, W, ov) in enumerate(_case_specs()):
        pat = PATTERNS[i % len(PATTERNS)]
        tag = "_".join(f"{k}{v:g}" for k, v in sorted(ov.items()))
        out.append((f"{i:02d}_{pat}_{B}x{H}x{W}_{tag}", *_inputs(pat, 7 * i, B, H, W), params_of(ov)))
    return tuple(out)


def references_for(image, alpha, params):
    """(reference in fp64, d32)"""
    r64 = reference(image, alpha, *params, dtype=np.float64)
    d32 = max(float(np.abs(reference(image, alpha, *params, dtype=np.float32, variant=v) - r64).max()) for v in (0, 1))
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
    line = f"[temporal] {name}: d32 = {d32:.3e} tol = {tol:.3e} d = {d:.3e} ratio = {d / max(d32, 1e-30):.2f}"
    print(line)
    if report is not None:
        report.append(line)
    assert d <= tol, line


def check(smooth, to_tensor, report=None):
    """smooth(image, alpha, radius, patch, color_tolerance, strength, max_change, clip_len) -> alpha on tensors made by `to_tensor` from CPU tensors;
    every case."""
    for name, image, alpha, params in cases():
        out = smooth(to_tensor(torch.from_numpy(image)), to_tensor(torch.from_numpy(alpha)), *params)
        compare(name, out, _references(name), report)


def offset_copy(t):
    """A contiguous copy of the CPU tensor t that starts 4 bytes off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype)
    k = 1 + (-(buf.data_ptr() // 4) % 4)              # element k is 16-byte aligned + 4 bytes
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---- what the call is for ---------------------------------------------------------------------------------------------------------------
PURPOSE = (2, 1, 0.1, 1.0, 1.0, 0)          # (radius, patch, color_tolerance, strength, max_change, clip_len)


@functools.lru_cache(maxsize=None)
def purpose_scene():
    """(image [8,96,128,3], true alpha, observed alpha): moving_disk at 3 pixels per frame, fixed seed."""
    return moving_disk(1234, 8, 96, 128, speed=3.0, noise=0.01, jitter=0.08)


def flicker(alpha, true):
    err = np.asarray(alpha, np.float64) - np.asarray(true, np.float64)
    return float(np.abs(err[1:] - err[:-1]).mean())


def check_purpose(smoothed, what):
    """flicker <= 0.5 x the observed alpha's, mean |out - true| <= 1.05 x observed, max |out - true| <= observed max + 0.01."""
    _, true, obs = purpose_scene()
    out = np.asarray(smoothed, np.float64).reshape(true.shape)
    e_out, e_obs = np.abs(out - true), np.abs(obs.astype(np.float64) - true)
    f_out, f_obs = flicker(out, true), flicker(obs, true)
    line = (f"[temporal] purpose ({what}): flicker {f_obs:.3e} -> {f_out:.3e} ({f_out / f_obs:.3f} x), mean {e_obs.mean():.3e} -> {e_out.mean():.3e} "
            f"({e_out.mean() / e_obs.mean():.3f} x), max {e_obs.max():.4f} -> {e_out.max():.4f}")
    print(line)
    assert f_out <= 0.5 * f_obs and e_out.mean() <= 1.05 * e_obs.mean() and e_out.max() <= e_obs.max() + 0.01, line
    return line
