"""Shared by tests/test_node_harmonize_cpu.py, tests/test_emu_harmonize.py and tests/test_gpu_harmonize.py: the harmonize cases, the exact-statistics case,
the purpose scenes, and a numpy reference of the function defined in include/sdmatte.h (sdm_harmonize) that shares no code with the kernels
(csrc/k_harmonize.h) or with the torch restatement (sdmatte_nodes.harmonize_map / harmonize_cutout).  The reference is callable
  in fp64     moments by the two-pass centred form, the blur as a direct double loop over (j, i) with the weight w_j w_i (`fast64`: separable, for the one
              larger GPU case, where the double loop costs seconds);
  in fp32, variant 0   per-pixel terms in fp32, summed sequentially in fp32 over consecutive runs of 4096 pixels of an image; separable blur, rows first;
  in fp32, variant 1   per-pixel terms in fp32, one np.sum partial per image row; the blur as the direct double loop;
both fp32 variants finalise in fp64 from the raw moments, as the summation contract says, and round the map to fp32.

Tolerance of `compare`, per case and for out, fg_out and map_out each: max(4 * d32, 2**-20) on the max abs difference to reference(fp64).
  * d32 is the larger distance to reference(fp64) of the two fp32 variants.  It is computed here, never taken from the code under test.
  * 4x: another fp32 evaluation differs in summation order, FMA contraction of the blur sums and the grouping of the partials, each a perturbation of the
    size of fp32 rounding (the margin of defocus_suite.py, temporal_suite.py, guided_suite.py and foreground_suite.py, for the same reasons).
  * floor 2**-20 = 8 ulp of 1.0, for constant inputs.
  * The function has one discontinuity, at Wf = SDM_HZ_MIN_WEIGHT = 1: `cases` asserts that every case has Wf < 0.5 or Wf > 2.
The strengths and the sigma cross the C ABI as floats, so the reference rounds them the same way first: d32 measures arithmetic only."""
import functools

import numpy as np
import torch

RUN = 4096                  # SDM_HZ_RUN
VAR_FLOOR = 2.0 ** -20      # SDM_HZ_VAR_FLOOR
MAX_GAIN = 4.0              # SDM_HZ_MAX_GAIN
MIN_WEIGHT = 1.0            # SDM_HZ_MIN_WEIGHT
DEFAULTS = (0.6, 0.8, 0.5, 0.5, 6.0)      # luma, chroma, contrast, wrap strength, wrap sigma

# the projectors of the opponent coordinates (l, p, q) and the directions of their unit steps in RGB
P = np.array([[[1, 1, 1], [1, 1, 1], [1, 1, 1]], [[1.5, -1.5, 0], [-1.5, 1.5, 0], [0, 0, 0]], [[.5, .5, -1], [.5, .5, -1], [-1, -1, 2]]], np.float64) / 3.0
K = np.array([[1, 1, 1], [.5, -.5, 0], [1 / 3, 1 / 3, -2 / 3]], np.float64)


# ---- reference --------------------------------------------------------------------------------------------------------------------------
def sanitise_alpha(alpha):
    a = np.asarray(alpha, np.float32)
    a = np.where(np.isnan(a), np.float32(0), a)
    return np.minimum(np.maximum(a, np.float32(0)), np.float32(1)).astype(np.float32)


def opponent(c):
    """[..., 3] -> [..., 3] = (l, p, q), in the dtype of c"""
    t = c.dtype.type
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    return np.stack([((r + g) + b) / t(3), r - g, (r + g) / t(2) - b], -1)


def _run_sums(terms):
    """terms [n, k] fp32 -> sequential fp32 sums over consecutive runs of RUN rows, then their fp64 total [k]"""
    tot = np.zeros(terms.shape[1], np.float64)
    for s in range(0, terms.shape[0], RUN):
        tot += np.cumsum(terms[s:s + RUN], axis=0, dtype=np.float32)[-1].astype(np.float64)      # (cumsum accumulates in order)
    return tot


def moments(F, a, Bg, dtype, variant):
    """one image: F, Bg [H,W,3], a [H,W] in `dtype` -> (Wf, mf[3], vf[3], mb[3], vb[3]) in fp64"""
    H, W = a.shape
    oF, oB = opponent(F), opponent(Bg)
    if dtype == np.float64:
        Wf = a.sum()
        if Wf <= 0:
            mf, vf = np.zeros(3), np.zeros(3)
        else:
            mf = (a[..., None] * oF).sum((0, 1)) / Wf
            vf = (a[..., None] * (oF - mf) ** 2).sum((0, 1)) / Wf
        mb = oB.mean((0, 1))
        vb = ((oB - mb) ** 2).mean((0, 1))
        return float(Wf), mf, vf, mb, vb
    ao = a[..., None] * oF
    terms = np.concatenate([a[..., None], ao, ao * oF, oB, oB * oB], -1)
    assert terms.dtype == np.float32
    if variant == 0:
        S = _run_sums(terms.reshape(H * W, 13))
    else:
        S = np.sum(terms, axis=1, dtype=np.float32).astype(np.float64).sum(0)
    n = float(H * W)
    Wf = S[0]
    mf = S[1:4] / Wf if Wf > 0 else np.zeros(3)
    vf = S[4:7] / Wf - mf * mf if Wf > 0 else np.zeros(3)
    mb = S[7:10] / n
    vb = S[10:13] / n - mb * mb
    return float(Wf), mf, vf, mb, vb


def map_from_moments(Wf, mf, vf, mb, vb, luma, chroma, contrast):
    """fp64 (M [3,3], t [3])"""
    M, t = np.eye(3), np.zeros(3)
    if Wf < MIN_WEIGHT or (luma == 0 and chroma == 0):
        return M, t
    for c, s in enumerate((luma, chroma, chroma)):
        rho = min(max(np.sqrt((max(vb[c], 0.0) + VAR_FLOOR) / (max(vf[c], 0.0) + VAR_FLOOR)), 1.0 / MAX_GAIN), MAX_GAIN)      # (the header's clamp at 0)
        g = 1.0 + contrast * s * (rho - 1.0)
        h = mf[c] * (1.0 - g) + s * (mb[c] - mf[c])
        M = M + (g - 1.0) * P[c]
        t = t + h * K[c]
    return M, t


def wrap_weights(sigma):
    """(r, w[2r + 1]) : computed in double, normalised, rounded to fp32"""
    s = float(np.float32(sigma))
    r = int(np.ceil(3.0 * s))
    i = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(i * i) / (2.0 * s * s))
    return r, (g / g.sum()).astype(np.float32)


def _shifted(X, dy, dx):
    """X [B,H,W,C] read at (y + dy, x + dx), 0 beyond the frame"""
    B, H, W, _ = X.shape
    out = np.zeros_like(X)
    ya, yb, xa, xb = max(0, -dy), H - max(0, dy), max(0, -dx), W - max(0, dx)
    if ya < yb and xa < xb:
        out[:, ya:yb, xa:xb] = X[:, ya + dy:yb + dy, xa + dx:xb + dx]
    return out


def blur(X, sigma, separable):
    r, w = wrap_weights(sigma)
    w = w.astype(X.dtype)
    if separable:
        T = np.zeros_like(X)
        for i in range(-r, r + 1):
            T += w[i + r] * _shifted(X, 0, i)
        out = np.zeros_like(X)
        for j in range(-r, r + 1):
            out += w[j + r] * _shifted(T, j, 0)
        return out
    out = np.zeros_like(X)
    for j in range(-r, r + 1):
        if abs(j) >= X.shape[1]:
            continue
        for i in range(-r, r + 1):
            if abs(i) < X.shape[2]:
                out += (w[j + r] * w[i + r]) * _shifted(X, j, i)
    return out


def reference(fg, alpha, bg, luma, chroma, contrast, wrap, sigma, dtype=np.float64, variant=0, fast64=False, clamp=True):
    """fg [B,H,W,3], alpha [B,H,W], bg [1 or B,H,W,3] -> (out, fg_out, map [B,12]) in `dtype`.  clamp=False: F' before its clamp takes the place of
    fg_out (the purpose scene asserts that it clamps nothing)."""
    luma, chroma, contrast, wrap = (float(np.float32(v)) for v in (luma, chroma, contrast, wrap))
    F = np.asarray(fg, np.float32).astype(dtype)
    a = sanitise_alpha(alpha).astype(dtype)
    Bg = np.asarray(bg, np.float32).astype(dtype)
    B = F.shape[0]
    if Bg.shape[0] == 1:
        Bg = np.repeat(Bg, B, 0)
    maps = np.zeros((B, 12), dtype)
    Fp = np.zeros_like(F)
    for b in range(B):
        M, t = map_from_moments(*moments(F[b], a[b], Bg[b], dtype, variant), luma, chroma, contrast)
        M, t = M.astype(dtype), t.astype(dtype)      # (rounded to fp32 at the end in the fp32 variants)
        maps[b, :9], maps[b, 9:] = M.reshape(9), t
        for k in range(3):
            Fp[b, ..., k] = ((t[k] + M[k, 0] * F[b, ..., 0]) + M[k, 1] * F[b, ..., 1]) + M[k, 2] * F[b, ..., 2]
    if not clamp:
        return None, Fp, maps
    one, zero = dtype(1), dtype(0)
    Fp = np.minimum(np.maximum(Fp, zero), one)
    if wrap > 0:
        v = one - a
        X = np.concatenate([v[..., None] * Bg, v[..., None]], -1)
        Wm = blur(X, sigma, separable=fast64 if dtype == np.float64 else variant == 0)
        Fp = np.minimum(np.maximum(Fp + dtype(wrap) * (Wm[..., :3] - Wm[..., 3:] * Fp), zero), one)
    out = a[..., None] * Fp + (one - a[..., None]) * Bg
    assert out.dtype == dtype and Fp.dtype == dtype and maps.dtype == dtype
    return out, Fp, maps


def subject_weight(alpha):
    """Wf per image in fp64"""
    return sanitise_alpha(alpha).astype(np.float64).sum((1, 2))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
PATTERNS = ["soft", "hard", "const0", "const1", "noise", "dirty"]


def _texture(rng, B, H, W, base, amp):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for b in range(B):
        ph = rng.uniform(0.0, 6.0, 3)
        waves = np.stack([np.sin(x / 5.0 + ph[0]) * np.cos(y / 7.0), np.sin(y / 4.0 + x / 9.0 + ph[1]), np.cos((x + y) / 6.0 + ph[2])], -1)
        out.append(np.clip(np.asarray(base) + amp * waves + rng.uniform(-amp / 2, amp / 2, (H, W, 3)), 0.0, 1.0))
    return np.stack(out)


def make_alpha(pattern, rng, B, H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    alpha = np.zeros((B, H, W))
    for b in range(B):
        cy, cx = (0.45 + 0.05 * b) * H, (0.55 - 0.05 * b) * W
        d = np.sqrt((y - cy) ** 2 + (x - cx) ** 2)
        if pattern in ("soft", "dirty"):
            alpha[b] = np.clip(0.5 - (d - 0.3 * max(H, W)) / 3.0, 0.0, 1.0)
        elif pattern == "hard":
            alpha[b] = (d <= 0.35 * max(H, W)).astype(np.float64)
        elif pattern == "const1":
            alpha[b] = 1.0
        elif pattern == "noise":
            alpha[b] = rng.uniform(size=(H, W))
    if pattern == "dirty":               # NaN and values outside [0, 1] sprinkled in
        pick = rng.uniform(size=alpha.shape)
        alpha[pick < 0.03] = np.nan
        alpha[(pick >= 0.03) & (pick < 0.06)] = -0.5
        alpha[(pick >= 0.06) & (pick < 0.09)] = 1.5
    return alpha


def inputs(pattern, seed, B, H, W, bg_batch=None, special=None):
    """(fg, alpha, bg): a warm subject, a cooler scene, different content per image.  special "tiny": the whole subject is 0.3 of one pixel;
    "flat": the subject has one colour (vf = 0)."""
    rng = np.random.default_rng(seed + 9000)
    fg = _texture(rng, B, H, W, (0.6, 0.5, 0.35), 0.2)
    bg = _texture(rng, B if bg_batch is None else bg_batch, H, W, (0.35, 0.45, 0.6), 0.3)
    alpha = make_alpha(pattern, rng, B, H, W)
    if special == "tiny":
        alpha[:] = 0.0
        alpha[:, H // 2, W // 2] = 0.3
    elif special == "flat":
        fg[:] = np.array([0.7, 0.4, 0.2])
    c = lambda t: np.ascontiguousarray(t, np.float32)
    return c(fg), c(alpha), c(bg)


def _case_specs():
    """(H, W, sigma, pattern, bg_batch, (luma, chroma, contrast, wrap), special), B = 3.  W crosses the 64-column tiles and the 256-pixel segments
    (1, 37, 70, 130, 260), H lies below r, makes H W smaller than one run or no multiple of 4096 (67 x 130, 40 x 260), sigma gives r = 1 .. 48, larger
    than the image too; every stage on and off; a subject of less than one pixel; a flat-coloured subject (rho at its clamp)."""
    on = (0.6, 0.8, 0.5, 0.5)
    return [(67, 130, 2.0, "soft", 3, on, None), (40, 260, 6.0, "hard", 1, on, None), (9, 37, 16.0, "noise", 3, on, None), (1, 70, 2.0, "dirty", 1, on, None),
            (40, 1, 0.3, "soft", 3, on, None), (40, 130, 16.0, "dirty", 1, (1.0, 1.0, 1.0, 1.0), None), (9, 260, 6.0, "const0", 3, on, None),
            (40, 70, 2.0, "const1", 1, on, None), (67, 37, 6.0, "noise", 3, (0.0, 0.0, 0.5, 0.7), None), (40, 130, 6.0, "soft", 1, (0.6, 0.8, 0.5, 0.0), None),
            (9, 70, 6.0, "dirty", 3, (0.0, 0.0, 0.0, 0.0), None), (67, 130, 0.3, "hard", 1, (0.7, 0.0, 1.0, 0.3), None),
            (40, 260, 2.0, "noise", 3, (0.0, 0.9, 0.0, 1.0), None), (40, 70, 2.0, "const0", 1, on, "tiny"), (67, 70, 6.0, "soft", 3, (0.5, 0.5, 1.0, 0.5), "flat"),
            (1, 37, 0.3, "const1", 1, on, None), (67, 260, 2.0, "soft", 1, on, None)]


@functools.lru_cache(maxsize=None)
def cases():
    """((name, fg, alpha, bg, (luma, chroma, contrast, wrap, sigma)), ...)"""
    out = []
    for i, (H, W, sigma, pat, bgb, (lu, ch, co, wr), special) in enumerate(_case_specs()):
        fg, alpha, bg = inputs(pat, 11 * i, 3, H, W, bgb, special)
        wf = subject_weight(alpha)
        assert np.all((wf < 0.5) | (wf > 2.0)), (i, wf)          # no case at the discontinuity Wf = 1
        name = f"{i:02d}_{pat}{'_' + special if special else ''}_3x{H}x{W}_bg{bgb}_s{sigma:g}_l{lu:g}c{ch:g}k{co:g}w{wr:g}"
        out.append((name, fg, alpha, bg, (lu, ch, co, wr, sigma)))
    return tuple(out)


def references_for(fg, alpha, bg, params, fast64=False):
    """((out, fg_out, map) in fp64, (d32 of out, of fg_out, of map))"""
    r64 = reference(fg, alpha, bg, *params, dtype=np.float64, fast64=fast64)
    d32 = [0.0, 0.0, 0.0]
    for v in (0, 1):
        if fast64 and v == 1:
            continue                     # (the larger case: the direct double loop costs seconds; variant 0 has the sums of a real kernel)
        r32 = reference(fg, alpha, bg, *params, dtype=np.float32, variant=v)
        d32 = [max(d, float(np.abs(x.astype(np.float64) - y).max())) for d, x, y in zip(d32, r32, r64)]
    return r64, tuple(d32)


@functools.lru_cache(maxsize=None)
def _references(name):
    """Computed once per process and shared by every test that needs it."""
    _, fg, alpha, bg, params = next(c for c in cases() if c[0] == name)
    return references_for(fg, alpha, bg, params)


def tolerance(d32):
    return max(4.0 * d32, 2.0 ** -20)


def compare(name, got, refs, report=None):
    """got = (out, fg_out, map) as torch tensors on any device, against the references of a case, under the rule above."""
    r64, d32 = refs
    for what, g, r, d in zip(("out", "fg_out", "map"), got, r64, d32):
        tol = tolerance(d)
        g = g.detach().cpu()
        assert g.dtype == torch.float32 and tuple(g.shape) == r.shape, (name, what, g.dtype, tuple(g.shape))
        g = g.numpy()
        assert np.isfinite(g).all(), (name, what)
        diff = float(np.abs(g.astype(np.float64) - r).max())
        line = f"[harmonize] {name} {what}: d32 = {d:.3e} tol = {tol:.3e} d = {diff:.3e} ratio = {diff / max(d, 1e-30):.2f}"
        print(line)
        if report is not None:
            report.append(line)
        assert diff <= tol, line


def check(harmonize, to_tensor, report=None):
    """harmonize(fg, alpha, bg, luma, chroma, contrast, wrap, sigma) -> (out, fg_out, map) on tensors made by `to_tensor` from CPU tensors; every case."""
    for name, fg, alpha, bg, params in cases():
        got = harmonize(*(to_tensor(torch.from_numpy(t)) for t in (fg, alpha, bg)), *params)
        compare(name, got, _references(name), report)


def stages_on(params):
    """the launches of a call with these parameters, in order (include/sdmatte.h)"""
    lu, ch, _, wr, _ = params
    return (("hz_stats", "hz_finalize") if lu > 0 or ch > 0 else ()) + (("hz_rows", ) if wr > 0 else ()) + ("hz_compose", )


def expected_counts(param_list):
    out = {}
    for p in param_list:
        for k in stages_on(p):
            out[k] = out.get(k, 0) + 1
    return out


def offset_copy(t):
    """A contiguous copy of the CPU tensor t that starts 4 bytes off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype)
    k = 1 + (-(buf.data_ptr() // 4) % 4)              # element k is 16-byte aligned + 4 bytes
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---- exact statistics -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_case():
    """(fg, alpha, bg, params, map64 [2,12], tol): grey F and Bg with values k / 8 and a in {0, 1} on 2 x 67 x 130 pixels (3 runs per image, the last one
    ragged).  Every per-pixel term is a multiple of 1 / 64 below 1 and there are fewer than 2^17 pixels, so every fp32 sum is exact in any order: the
    map of an implementation differs from reference(fp64) by the rounding of its fp64 finalisation to fp32 only.  tol = 4 ulp of fp32 at 1.0 (no entry
    of these maps exceeds 2 in magnitude... see the assertion).  Flipping one pixel's alpha moves the reference map by more than 100 tol, so a dropped
    or doubled pixel cannot pass."""
    rng = np.random.default_rng(77)
    B, H, W = 2, 67, 130
    fg = np.repeat(rng.integers(0, 9, (B, H, W, 1)) / 8.0, 3, -1).astype(np.float32)
    bg = np.repeat(rng.integers(2, 8, (B, H, W, 1)) / 8.0, 3, -1).astype(np.float32)
    alpha = (rng.uniform(size=(B, H, W)) < 0.2).astype(np.float32)
    params = (1.0, 1.0, 1.0, 0.0, 6.0)
    m64 = reference(fg, alpha, bg, *params)[2]
    tol = 4.0 * float(np.spacing(np.float32(1.0)))
    assert float(np.abs(m64).max()) < 2.0
    for b in range(B):                   # the most telling pixel of each image: the last one (it lies in the ragged run), set to the far value
        a2, f2 = alpha.copy(), fg.copy()
        a2[b, -1, -1] = 1.0 - a2[b, -1, -1]
        f2[b, -1, -1] = 1.0
        moved = float(np.abs(reference(f2, a2, bg, *params)[2][b] - reference(f2, alpha, bg, *params)[2][b]).max())
        assert moved > 100.0 * tol, (b, moved, tol)
    return fg, alpha, bg, params, m64, tol


def check_exact(map_out, who):
    fg, alpha, bg, params, m64, tol = exact_case()
    d = float(np.abs(np.asarray(map_out, np.float64).reshape(m64.shape) - m64).max())
    line = f"[harmonize] exact statistics ({who}): max |map - reference(fp64)| = {d:.3e}, 4 ulp = {tol:.3e}"
    print(line)
    assert d <= tol, line
    return line


# ---- what the call is for ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def match_scene():
    """(fg, alpha, bg, params): a warm textured subject (a soft disc) over a cool textured scene, 96 x 160, luma = chroma = contrast = 1, no wrap.  The
    amplitudes are small enough for reference(fp64) to clamp no pixel with a > 0 (asserted), so the mapped moments are the scene's, and large enough
    for the variance floor to matter less than 1e-3 (at an amplitude of 0.05 it moved the variances by 1.6e-3)."""
    H, W = 96, 160
    rng = np.random.default_rng(5)
    fg = _texture(rng, 1, H, W, (0.62, 0.5, 0.38), 0.12)
    bg = _texture(rng, 1, H, W, (0.38, 0.5, 0.62), 0.15)
    alpha = make_alpha("soft", rng, 1, H, W)
    fg, alpha, bg = (np.ascontiguousarray(t, np.float32) for t in (fg, alpha, bg))
    params = (1.0, 1.0, 1.0, 0.0, 6.0)
    raw = reference(fg, alpha, bg, *params, clamp=False)[1]
    inside = raw[sanitise_alpha(alpha) > 0]
    assert inside.min() > 0.0 and inside.max() < 1.0, (inside.min(), inside.max())
    return fg, alpha, bg, params


def weighted_opponent_moments(colours, weight):
    o = opponent(np.asarray(colours, np.float64))
    w = np.asarray(weight, np.float64)[..., None]
    m = (w * o).sum((0, 1, 2)) / w.sum()
    return m, (w * (o - m) ** 2).sum((0, 1, 2)) / w.sum()


def check_match_purpose(fg_out, who):
    """fg_out = the call on match_scene().  Before: the a-weighted opponent means of F differ from the scene's by more than 0.1 in at least two
    coordinates.  After: the means of fg_out equal the scene's - to twice the tolerance of fg_out on this scene (an opponent coordinate is a combination
    of colours with absolute weights summing to at most 2, and a mean of errors is no larger than the largest) - and the variances agree to 1e-3
    relative (1e-4 in fp64: the variance floor's doing)."""
    fg, alpha, bg, params = match_scene()
    a = sanitise_alpha(alpha)
    mb, vb = weighted_opponent_moments(bg, np.ones_like(a))
    m0, _ = weighted_opponent_moments(fg, a)
    assert int((np.abs(m0 - mb) > 0.1).sum()) >= 2, (m0, mb)
    _, d32 = references_for(fg, alpha, bg, params)
    tol = 2.0 * tolerance(d32[1]) + 1e-9
    m1, v1 = weighted_opponent_moments(np.asarray(fg_out, np.float32).reshape(fg.shape), a)
    line = (f"[harmonize] match purpose ({who}): means before {np.round(m0, 4)}, scene {np.round(mb, 4)}, after - scene {np.abs(m1 - mb).max():.3e} "
            f"(tol {tol:.3e}); variance ratio - 1: {np.abs(v1 / vb - 1).max():.3e}")
    print(line)
    assert np.all(np.abs(m1 - mb) <= tol), line
    assert np.all(np.abs(v1 / vb - 1.0) <= 1e-3), line
    return line


WRAP_SIGMA, WRAP_X0, WRAP_X1 = 2.0, 24, 72


@functools.lru_cache(maxsize=None)
def wrap_scene():
    """(fg, alpha, bg, params): a black subject (F = 0, a = 1 on columns 24 .. 71 of every row, 0 elsewhere) over a 40 x 96 scene whose right half is
    white and whose left half is black; wrap only (strength 1, sigma 2, r = 6)."""
    H, W = 40, 96
    fg = np.zeros((1, H, W, 3), np.float32)
    alpha = np.zeros((1, H, W), np.float32)
    alpha[:, :, WRAP_X0:WRAP_X1] = 1.0
    bg = np.zeros((1, H, W, 3), np.float32)
    bg[:, :, W // 2:] = 1.0
    return fg, alpha, bg, (0.0, 0.0, 0.0, 1.0, WRAP_SIGMA)


def check_wrap_purpose(fg_out, who):
    """The scene's light reaches the subject's right edge (fg_out > 0 on its last column), nothing reaches its left edge (exactly 0: the visible
    background there is black), it does not increase inwards, and it is exactly 0 further than r from the visible background (identity 4, in pixels)."""
    fg, alpha, bg, params = wrap_scene()
    r = wrap_weights(WRAP_SIGMA)[0]
    f = np.asarray(fg_out, np.float32).reshape(fg.shape)[0]
    sub = f[:, WRAP_X0:WRAP_X1]
    line = f"[harmonize] wrap purpose ({who}): right edge min {sub[:, -1].min():.3e}, left edge max {np.abs(sub[:, 0]).max():.3e}, r = {r}"
    print(line)
    assert np.all(sub[:, -1] > 0.0), line
    assert np.all(sub[:, :WRAP_X1 - WRAP_X0 - r] == 0.0), line
    assert np.all(sub[:, -r:] > 0.0), line                      # every column within r of the visible white carries some of it
    assert np.all(np.diff(sub, axis=1) >= 0.0), line            # non-increasing inwards (leftwards)
    return line
