"""Shared by tests/test_node_motion_cpu.py, tests/test_emu_motion.py and tests/test_gpu_motion.py: the cases of the motion-compensated temporal smoothing,
the translation and purpose scenes, and a numpy reference of the function defined in include/sdmatte.h (sdm_smooth_alpha_motion) that shares no code with
the kernel (csrc/k_motion.h) or with the torch restatement (sdmatte_nodes.temporal_smooth_alpha_motion): explicit loops over k, over the displacements and
over the patch offsets, callable in fp64 and fp32.

The function contains a discrete choice (the best displacement), so it is not continuous where the two best costs meet: an fp32 evaluation may choose the
other one there and sample another alpha.  Such pixels are UNDECIDED and are excluded from the comparison of values (they must still be finite and in
[0, 1]): a pixel of frame t is undecided if, for some neighbour, the best and the second-best eligible cost of the fp64 evaluation satisfy
(C2 - C1) / max(C2, 1e-30) < 1e-4 and the smaller of their two D is below tau2 (otherwise both weights are exactly 0 and the flip cannot matter).
  * 1e-4: an fp32 evaluation of C (up to 25 x 3 squared differences, one division, one product, one sum) is good to about 30 * 2**-24 = 2e-6 relative;
    1e-4 is 50 times that.
  * The share of undecided pixels of a case is at most 0.5 % (asserted on the reference alone in tests/test_node_motion_cpu.py): a case that breaks
    this is replaced, not excused.
Tolerance of `compare` on the other pixels, per case: max(4 * d32, 2**-20) on the max abs difference to reference(fp64), the rule of temporal_suite.py.
d32 is the larger distance to reference(fp64), on those pixels, of two fp32 evaluations of the reference that differ in summation order (row-major patch
sums, k and candidates ascending; separable patch sums, k and candidates descending).  It is computed here, never taken from the code under test."""
import functools

import numpy as np
import torch

import temporal_suite as TS
from temporal_suite import _patch_sum, cut_scene, moving_disk, offset_copy, sanitise_alpha      # noqa: F401  (re-exported for the tests)

REL_GAP = 1e-4
MAX_UNDECIDED_SHARE = 0.005


# ---- reference --------------------------------------------------------------------------------------------------------------------------
def _shifted(src, dy, dx, fill=0):
    """(out, ok): out[y, x] = src[y + dy, x + dx] where that pixel exists (ok), `fill` elsewhere; src is [H, W] or [H, W, C]"""
    H, W = src.shape[:2]
    out = np.full_like(src, fill)
    ok = np.zeros((H, W), bool)
    ya, yb, xa, xb = max(0, -dy), H - max(0, dy), max(0, -dx), W - max(0, dx)
    if ya < yb and xa < xb:
        out[ya:yb, xa:xb] = src[ya + dy:yb + dy, xa + dx:xb + dx]
        ok[ya:yb, xa:xb] = True
    return out, ok


def reference(image, alpha, radius, patch, search, color_tolerance, motion_penalty, strength, max_change, clip_len, dtype=np.float64, variant=0):
    """image [B,H,W,3], alpha [B,H,W] -> (smoothed alpha [B,H,W] in `dtype`, undecided [B,H,W] bool).  variant 0: row-major patch sums, k and candidates
    ascending; 1: separable patch sums, k and candidates descending (the choice rule does not depend on the order of evaluation)."""
    if search == 0:
        out = TS.reference(image, alpha, radius, patch, color_tolerance, strength, max_change, clip_len, dtype=dtype, variant=variant)
        return out, np.zeros(out.shape, bool)
    one, zero = dtype(1), dtype(0)
    t32 = np.float32(color_tolerance)
    tau2_32 = np.float32(t32 * t32)
    pt = dtype(np.float32(np.float32(motion_penalty) * tau2_32))
    tau2, strength, max_change = dtype(tau2_32), dtype(np.float32(strength)), dtype(np.float32(max_change))
    img = np.asarray(image, np.float32).astype(dtype)
    a = sanitise_alpha(alpha).astype(dtype)
    B, H, W = a.shape
    L = int(clip_len) if clip_len else B
    out = np.empty_like(a)
    undecided = np.zeros(a.shape, bool)
    ks = [-j for j in range(1, radius + 1)] + list(range(1, radius + 1))          # the order of the filter's sums is part of the definition ...
    cands = [(dy, dx) for dy in range(-search, search + 1) for dx in range(-search, search + 1)]
    if variant:
        cands = cands[::-1]                                                       # ... the order in which candidates are looked at is not
    inf = dtype(np.inf)
    for t in range(B):
        num, den = a[t].copy(), np.ones((H, W), dtype)
        for k in ks:
            s = t + k
            if s < 0 or s >= B or s // L != t // L:
                continue
            got = np.zeros((H, W), bool)
            bC, bD, bA = np.zeros((H, W), dtype), np.zeros((H, W), dtype), np.zeros((H, W), dtype)
            bdd, bdy, bdx = np.zeros((H, W), int), np.zeros((H, W), int), np.zeros((H, W), int)
            c1, c2, d1, d2 = np.full((H, W), inf), np.full((H, W), inf), np.full((H, W), inf), np.full((H, W), inf)      # the two smallest costs, their D
            for dy, dx in cands:
                Isd, ok = _shifted(img[s], dy, dx)
                if not ok.any():
                    continue
                As, _ = _shifted(a[s], dy, dx)
                d = Isd - img[t]
                with np.errstate(invalid="ignore", over="ignore"):
                    e = np.where(ok, (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], zero)
                    n = _patch_sum(ok.astype(dtype), patch, False)
                    D = _patch_sum(e, patch, bool(variant)) / (dtype(3) * np.maximum(n, one))
                    dd = dy * dy + dx * dx
                    C = D + pt * dtype(dd)
                    elig = ok & (C == C)
                    better = elig & (~got | (C < bC) | ((C == bC) & ((dd < bdd) | ((dd == bdd) & ((dy < bdy) | ((dy == bdy) & (dx < bdx)))))))
                    first = elig & (C < c1)
                    second = elig & ~first & (C < c2)
                c2, d2 = np.where(first, c1, np.where(second, C, c2)), np.where(first, d1, np.where(second, D, d2))
                c1, d1 = np.where(first, C, c1), np.where(first, D, d1)
                # (a candidate that ties with the best lands in c2: gap 0)
                bC, bD, bA = np.where(better, C, bC), np.where(better, D, bD), np.where(better, As, bA)
                bdd, bdy, bdx = np.where(better, dd, bdd), np.where(better, dy, bdy), np.where(better, dx, bdx)
                got |= better
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                gap = (c2 - c1) / np.maximum(c2, dtype(1e-30))
                undecided[t] |= np.isfinite(c2) & (gap < REL_GAP) & (np.minimum(d1, d2) < tau2)
            u = one - bD / tau2
            u = np.where(u > zero, u, zero)
            w = np.where(got, strength * (one - dtype(abs(k)) / dtype(radius + 1)) * (u * u), zero)
            num = num + w * bA
            den = den + w
        f = num / den
        out[t] = np.minimum(np.maximum(a[t] + np.minimum(np.maximum(f - a[t], -max_change), max_change), zero), one)
    assert out.dtype == dtype
    return out, undecided


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
DEFAULTS = {"radius": 2, "patch": 1, "search": 4, "color_tolerance": 0.1, "motion_penalty": 0.02, "strength": 1.0, "max_change": 1.0, "clip_len": 0}
KEYS = ("radius", "patch", "search", "color_tolerance", "motion_penalty", "strength", "max_change", "clip_len")
PATTERNS = ["moving", "static", "cut", "noise", "const0", "dirty"]


def inputs(pattern, seed, B, H, W):
    return TS._inputs(pattern, seed, B, H, W)


def _case_specs():
    """(B, H, W, overrides).  The kernel's tile is (64 - 2 patch) columns x 16 rows: widths of 70, 130 and 132 and heights of 33 and 37 cross a seam."""
    specs = [(3, 33, 70, {"search": 1}), (3, 33, 70, {"search": 2}), (4, 33, 70, {}),
             (3, 20, 40, {"search": 8}), (2, 20, 40, {"search": 8, "radius": 1, "motion_penalty": 0.0})]      # the emulator is slow: search 8 twice only
    specs += [(3, 33, 70, {"patch": 0}), (3, 37, 72, {"patch": 2}), (3, 20, 132, {"patch": 2, "search": 3})]
    specs += [(2, 20, 40, {"radius": 1}), (3, 20, 40, {"radius": 1}), (2, 33, 70, {}), (5, 20, 40, {}),
              (4, 20, 40, {"radius": 4, "search": 2}), (9, 9, 40, {"radius": 4, "search": 2})]
    specs += [(3, 33, 70, {"motion_penalty": 0.0}), (3, 33, 70, {"motion_penalty": 1.0})]
    specs += [(5, 20, 40, {"clip_len": c, "search": 2}) for c in (0, 1, 3)]                                  # 3: a ragged last clip
    specs += [(3, 1, 1, {}), (3, 1, 70, {}), (3, 37, 1, {"patch": 2}), (3, 3, 130, {}), (3, 33, 2, {"search": 3})]      # sides of 1 and below `search`
    specs += [(3, 9, 132, {}), (3, 9, 130, {"patch": 0})]                                                  # W % 4 == 0: the 16-byte load path
    specs += [(3, 20, 70, {"strength": 0.5}), (3, 20, 70, {"max_change": 0.05})]
    return specs


def params_of(overrides):
    p = dict(DEFAULTS, **overrides)
    return tuple(p[k] for k in KEYS)


@functools.lru_cache(maxsize=None)
def cases():
    """((name, image, alpha, (radius, patch, search, color_tolerance, motion_penalty, strength, max_change, clip_len)), ...), the content patterns in turn."""
    out = []
    for i, (B, H, W, ov) in enumerate(_case_specs()):
        pat = PATTERNS[i % len(PATTERNS)]
        tag = "_".join(f"{k}{v:g}" for k, v in sorted(ov.items()))
        out.append((f"{i:02d}_{pat}_{B}x{H}x{W}_{tag}", *inputs(pat, 7 * i, B, H, W), params_of(ov)))
    return tuple(out)


def references_for(image, alpha, params):
    """(reference in fp64, undecided, d32 on the decided pixels)"""
    r64, und = reference(image, alpha, *params, dtype=np.float64)
    d32 = 0.0
    for v in (0, 1):
        r32, _ = reference(image, alpha, *params, dtype=np.float32, variant=v)
        diff = np.abs(r32 - r64)[~und]
        d32 = max(d32, float(diff.max()) if diff.size else 0.0)
    return r64, und, d32


@functools.lru_cache(maxsize=None)
def _references(name):
    """Computed once per process and shared by every test that needs it."""
    _, image, alpha, params = next(c for c in cases() if c[0] == name)
    return references_for(image, alpha, params)


def undecided_share(refs):
    return float(refs[1].mean())


def tolerance(d32):
    return max(4.0 * d32, 2.0 ** -20)


def compare(name, out, refs, report=None):
    """out (a torch tensor on any device) against the references of a case, under the rule above."""
    r64, und, d32 = refs
    tol = tolerance(d32)
    out = out.detach().cpu()
    assert out.dtype == torch.float32 and tuple(out.shape) == r64.shape, (name, out.dtype, tuple(out.shape))
    out = out.numpy()
    assert np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0, name
    diff = np.abs(out.astype(np.float64) - r64)[~und]
    d = float(diff.max()) if diff.size else 0.0
    line = (f"[motion] {name}: undecided {und.mean() * 100:.3f} % d32 = {d32:.3e} tol = {tol:.3e} d = {d:.3e} ratio = {d / max(d32, 1e-30):.2f}")
    print(line)
    if report is not None:
        report.append(line)
    assert d <= tol, line


def check(smooth, to_tensor, report=None):
    """smooth(image, alpha, radius, patch, search, color_tolerance, motion_penalty, strength, max_change, clip_len) -> alpha on tensors made by `to_tensor`
    from CPU tensors; every case."""
    for name, image, alpha, params in cases():
        out = smooth(to_tensor(torch.from_numpy(image)), to_tensor(torch.from_numpy(alpha)), *params)
        compare(name, out, _references(name), report)


# ---- a pure translation: reference-free -------------------------------------------------------------------------------------------------
TRANSLATION = (2, 1, 4, 0.1, 0.02, 1.0, 1.0, 0)          # (radius, patch, search, color_tolerance, motion_penalty, strength, max_change, clip_len)
TRANSLATION_MARGIN = 4 + 1 + 4                            # search + patch + 4


@functools.lru_cache(maxsize=None)
def translation_scene(B=5, H=36, W=44, step=(1, -2), seed=99):
    """(image [B,H,W,3], alpha [B,H,W]): a uniform-random texture and an arbitrary random alpha field, both moved by `step` = (dy, dx) pixels per frame:
    frame t + 1 at p + step shows what frame t shows at p."""
    rng = np.random.default_rng(seed)
    my, mx = abs(step[0]) * B, abs(step[1]) * B
    tex = rng.uniform(size=(H + 2 * my, W + 2 * mx, 3)).astype(np.float32)
    alf = rng.uniform(size=(H + 2 * my, W + 2 * mx)).astype(np.float32)
    image = np.stack([tex[my - step[0] * t:my - step[0] * t + H, mx - step[1] * t:mx - step[1] * t + W] for t in range(B)])
    alpha = np.stack([alf[my - step[0] * t:my - step[0] * t + H, mx - step[1] * t:mx - step[1] * t + W] for t in range(B)])
    return np.ascontiguousarray(image), np.ascontiguousarray(alpha)


def check_translation(smooth, to_tensor, what):
    """With search 4 every neighbour within radius 2 is found at D = 0 and shows the pixel's own alpha: |out - a| <= 2**-20 on the pixels at least
    search + patch + 4 from every border.  That the test can fail: the same call on the same frames with an alpha that does NOT move with the texture
    (every frame carries frame 0's field) samples other values along the same displacements and moves those pixels by more than 0.01 somewhere.
    (The same call with search 1 cannot serve as that counter-check: the true displacement (1, -2) is out of its reach, every other candidate of a
    uniform-random texture has D of about 1/6 >= tau2, all weights are exactly 0 and out equals a - which the correct function returns and a broken
    one might too.)"""
    image, alpha = translation_scene()
    m = TRANSLATION_MARGIN
    im, al = to_tensor(torch.from_numpy(image)), to_tensor(torch.from_numpy(alpha))
    out = smooth(im, al, *TRANSLATION).detach().cpu().numpy()
    d = float(np.abs(out - alpha)[:, m:-m, m:-m].max())
    still = np.ascontiguousarray(np.repeat(alpha[:1], alpha.shape[0], 0))
    moved = smooth(im, to_tensor(torch.from_numpy(still)), *TRANSLATION).detach().cpu().numpy()
    d1 = float(np.abs(moved - still)[:, m:-m, m:-m].max())
    line = f"[motion] translation ({what}): max |out - a| inside = {d:.3e} with the alpha moving along, {d1:.3e} with a still alpha"
    print(line)
    assert d <= 2.0 ** -20 and d1 > 0.01, line
    return line


# ---- what the call is for ---------------------------------------------------------------------------------------------------------------
PURPOSE = (2, 1, 4, 0.1, 0.02, 1.0, 1.0, 0)


@functools.lru_cache(maxsize=None)
def purpose_scene():
    """(image [8,96,128,3], true alpha, observed alpha): moving_disk at 2 pixels per frame, fixed seed."""
    return moving_disk(1234, 8, 96, 128, speed=2.0, noise=0.01, jitter=0.08)


@functools.lru_cache(maxsize=None)
def purpose_band():
    """[8,96,128] bool: at frame t, the pixels whose TRUE alpha changes by more than 0.05 to frame t - 1 or to frame t + 1 - what the moving edge sweeps."""
    true = purpose_scene()[1].astype(np.float64)
    step = np.abs(true[1:] - true[:-1]) > 0.05
    band = np.zeros(true.shape, bool)
    band[1:] |= step
    band[:-1] |= step
    return band


@functools.lru_cache(maxsize=None)
def purpose_existing():
    """The existing filter's fp64 reference on the same scene (same radius, patch, tolerance)."""
    image, _, obs = purpose_scene()
    return TS.reference(image, obs, PURPOSE[0], PURPOSE[1], PURPOSE[3], 1.0, 1.0, 0)


def band_flicker(alpha):
    """mean |err[t] - err[t - 1]| over t >= 1 and the pixels that are in the band at frame t"""
    true = purpose_scene()[1].astype(np.float64)
    err = np.asarray(alpha, np.float64).reshape(true.shape) - true
    return float(np.abs(err[1:] - err[:-1])[purpose_band()[1:]].mean())


def purpose_figures(alpha):
    """(band flicker, band mean error, largest error, whole-frame flicker)"""
    true = purpose_scene()[1].astype(np.float64)
    err = np.abs(np.asarray(alpha, np.float64).reshape(true.shape) - true)
    return band_flicker(alpha), float(err[purpose_band()].mean()), float(err.max()), TS.flicker(np.asarray(alpha).reshape(true.shape), true)


def check_purpose(smoothed, what):
    """band flicker <= 0.55 x the observed alpha's, band mean error <= 0.85 x the observed, largest error <= the observed largest, whole-frame flicker
    <= 0.95 x that of the existing filter's reference on the same scene."""
    obs = purpose_scene()[2]
    bf, bm, mx, ff = purpose_figures(smoothed)
    obf, obm, omx, _ = purpose_figures(obs)
    _, _, _, eff = purpose_figures(purpose_existing())
    line = (f"[motion] purpose ({what}): band flicker {obf:.4f} -> {bf:.4f} ({bf / obf:.3f} x), band mean error {obm:.4f} -> {bm:.4f} ({bm / obm:.3f} x), "
            f"largest error {omx:.3f} -> {mx:.3f}, flicker vs the existing filter {eff:.3e} -> {ff:.3e} ({ff / eff:.3f} x)")
    print(line)
    assert bf <= 0.55 * obf and bm <= 0.85 * obm and mx <= omx and ff <= 0.95 * eff, line
    return line
