"""Shared by tests/test_node_plate_cpu.py, tests/test_emu_plate.py and tests/test_gpu_plate.py: the clean-plate cases, the purpose scene, and a numpy
reference of the function defined in include/sdmatte.h (sdm_fill_background) that shares no code with the kernels (csrc/k_plate.h) or with the torch
restatement (sdmatte_nodes.clean_plate).  The reference works on whole levels with strided slices (a level padded to even sides with zero weights: a
missing child adds 0 to either sum) and gathers; it is callable in fp64 and fp32.  w_0 is always formed in fp32 first, because it is an input of the
contract (a == 0 must give exactly 1 and a >= alpha_cut exactly 0 in every evaluation); everything after it is in the given dtype.

Tolerance of `compare`, per case: max(4 * d32, 2**-20) on the max abs difference to reference(fp64).
  * d32 is the distance of reference(fp32) to reference(fp64).  It is computed here, never taken from the code under test.
  * The function has only convex combinations and one division per level by a sum of at most four weights, no cancellation: every level adds a few
    roundings of values in the colours' range, so d32 is a few 2**-24 times the number of levels (1e-7 to 3e-7 on these inputs).
  * 4x: another fp32 evaluation may differ in FMA contraction and division sequence, each a perturbation of the size of fp32 rounding (the margin of
    defocus_suite.py, temporal_suite.py, guided_suite.py and foreground_suite.py).
  * floor 2**-20 = 8 ulp of 1.0, for constant inputs.

Case sizes sit where the kernels can go wrong: sides of 1 and levels with missing children (1x1, 1x300, 300x1, 2x3), the boundary between the one-block
kernel and the tiled ones (32x32, 33x31), odd sizes at every level and a tile seam in both directions (37x70, 67x131, 129x257; tiles are 64 x 32),
W % 4 == 0 beyond the small kernel (both load paths: 96x132, 200x300), and 200x300 with a disc of radius 80, whose interior is filled from levels beyond
one fused group of three (S = 4: two pull and two push launches).

The purpose scene (200 x 300, a soft red disc of radius 60 over a background without red), measured with reference(fp64) at alpha_cut = 1/16 on the image
alone: the plate's error against the true background over the hole (g and b) is max 0.0675 and mean 0.0160, against max 0.1706 and mean 0.0606 for
filling the hole with the weighted mean colour: ratios of 0.40 and 0.26.  (0.022 of the subject's red is left in the hole there, from the pixels with
0 < a < 1/16; with a hard alpha, or with a clean bg plane, it is exactly 0.)"""
import functools

import numpy as np
import torch

ALPHA_CUT = 0.0625          # SDM_PLATE_ALPHA_CUT
MIN_CUT = 2.0 ** -10        # SDM_PLATE_MIN_CUT
LAUNCH_NAMES = ("plate_pull", "plate_small", "plate_push")


# ---- reference --------------------------------------------------------------------------------------------------------------------------
def sanitise(plane):
    a = np.asarray(plane, np.float32)
    a = np.where(np.isnan(a), np.float32(0), a)
    return np.minimum(np.maximum(a, np.float32(0)), np.float32(1)).astype(np.float32)


def weights0(alpha, hole, alpha_cut):
    """w_0 in fp32, whatever the dtype of the rest"""
    a = sanitise(alpha)
    if hole is not None:
        a = np.maximum(a, sanitise(hole))
    w = np.float32(1) - a / np.float32(alpha_cut)
    assert w.dtype == np.float32
    return np.minimum(np.maximum(w, np.float32(0)), np.float32(1))


def reference(image, alpha, bg, hole, alpha_cut, dtype=np.float64):
    """image [B,H,W,3], alpha [B,H,W], bg [B,H,W,3] or None, hole [B,H,W] or None -> the plate [B,H,W,3] in `dtype`"""
    one, zero, n, f = dtype(1), dtype(0), dtype(0.75), dtype(0.25)
    C = np.asarray(image if bg is None else bg, np.float32).astype(dtype)
    w = weights0(alpha, hole, alpha_cut).astype(dtype)[..., None]
    levels = [(C, w)]
    while C.shape[1] > 1 or C.shape[2] > 1:
        B, h, ww, _ = C.shape
        hn, wn = (h + 1) // 2, (ww + 1) // 2
        Cp, wp = np.zeros((B, 2 * hn, 2 * wn, 3), dtype), np.zeros((B, 2 * hn, 2 * wn, 1), dtype)
        Cp[:, :h, :ww], wp[:, :h, :ww] = C, w
        kids = [(wp[:, dy::2, dx::2], Cp[:, dy::2, dx::2]) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
        Sw = ((kids[0][0] + kids[1][0]) + kids[2][0]) + kids[3][0]
        Sc = ((kids[0][0] * kids[0][1] + kids[1][0] * kids[1][1]) + kids[2][0] * kids[2][1]) + kids[3][0] * kids[3][1]
        some = Sw > zero
        C = np.where(some, Sc / np.where(some, Sw, one), zero)
        w = np.minimum(one, Sw)
        levels.append((C, w))
    F = levels[-1][0]
    for C, w in reversed(levels[:-1]):
        h, ww = C.shape[1:3]
        hc, wc = F.shape[1:3]
        y, x = np.arange(h), np.arange(ww)
        ny, nx = y >> 1, x >> 1
        fy = np.clip(ny + np.where(y & 1, 1, -1), 0, hc - 1)
        fx = np.clip(nx + np.where(x & 1, 1, -1), 0, wc - 1)
        Fn, Ff = F[:, ny], F[:, fy]
        U = n * (n * Fn[:, :, nx] + f * Fn[:, :, fx]) + f * (n * Ff[:, :, nx] + f * Ff[:, :, fx])
        F = w * C + (one - w) * U
    assert F.dtype == dtype
    return F


def levels_beyond_small(H, W):
    """S of include/sdmatte.h: the number of levels with max(h, w) > 32, by halving"""
    S = 0
    while max(H, W) > 32:
        H, W, S = (H + 1) // 2, (W + 1) // 2, S + 1
    return S


def launches(H, W, calls=1):
    """{name: launches} of `calls` calls on H x W, as sdm_kernel_counts reports them (a name that never ran is absent)"""
    g = (levels_beyond_small(H, W) + 2) // 3
    return {k: v * calls for k, v in (("plate_pull", g), ("plate_small", 1), ("plate_push", g)) if v}


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
PATTERNS = ["soft", "hard", "const0", "const1", "noise", "dirty", "disc80"]


def _texture(rng, B, H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for b in range(B):
        ph = rng.uniform(0.0, 6.0, 3)
        base = np.stack([0.5 + 0.3 * np.sin(x / 5.0 + ph[0]) * np.cos(y / 7.0), 0.5 + 0.3 * np.sin(y / 4.0 + ph[1]), 0.5 + 0.3 * np.cos((x + y) / 6.0 + ph[2])], -1)
        out.append(np.clip(base + rng.uniform(-0.2, 0.2, (H, W, 3)), 0.0, 1.0))
    return np.stack(out)


def inputs(pattern, seed, B, H, W, with_bg=False, with_hole=False):
    """(image, alpha, bg or None, hole or None): colours in [0, 1], different content per image of the batch."""
    rng = np.random.default_rng(seed + 9000)
    image = _texture(rng, B, H, W)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    alpha = np.zeros((B, H, W))
    for b in range(B):
        cy, cx = (0.45 + 0.1 * b) * H, (0.55 - 0.1 * b) * W
        d = np.sqrt((y - cy) ** 2 + (x - cx) ** 2)
        if pattern in ("soft", "dirty"):
            alpha[b] = np.clip(0.5 - (d - 0.3 * max(min(H, W), 8)) / 3.0, 0.0, 1.0)
        elif pattern == "hard":
            alpha[b] = (d <= 0.3 * max(H, W)).astype(np.float64)
        elif pattern == "disc80":
            alpha[b] = (d <= 80.0).astype(np.float64)
        elif pattern == "const1":
            alpha[b] = 1.0
        elif pattern == "noise":
            alpha[b] = rng.uniform(size=(H, W)) ** 4
    if pattern == "dirty":               # NaN and values outside [0, 1] sprinkled in
        pick = rng.uniform(size=alpha.shape)
        alpha[pick < 0.03] = np.nan
        alpha[(pick >= 0.03) & (pick < 0.06)] = -0.5
        alpha[(pick >= 0.06) & (pick < 0.09)] = 1.5
    bg = _texture(rng, B, H, W) if with_bg else None
    hole = None
    if with_hole:                        # a second, smaller object off the subject's centre, soft, with a NaN and an out-of-range value of its own
        hole = np.zeros((B, H, W))
        for b in range(B):
            d = np.sqrt((y - 0.2 * H) ** 2 + (x - (0.25 + 0.1 * b) * W) ** 2)
            hole[b] = np.clip(0.5 - (d - 0.12 * max(H, W)) / 2.0, 0.0, 1.0)
        hole[:, H // 2, W // 3] = np.nan
        hole[:, H // 3, W // 2] = 1.5
    c = lambda t: None if t is None else np.ascontiguousarray(t, np.float32)
    return c(image), c(alpha), c(bg), c(hole)


def _case_specs():
    """(B, H, W, pattern, bg, hole, alpha_cut): see the module docstring for the sizes"""
    return [(1, 1, 1, "const0", False, False, 1.0), (2, 1, 300, "soft", True, False, 0.25), (2, 300, 1, "dirty", False, True, ALPHA_CUT),
            (2, 2, 3, "noise", True, True, MIN_CUT), (2, 32, 32, "soft", False, False, ALPHA_CUT), (2, 33, 31, "hard", True, False, 1.0),
            (3, 37, 70, "dirty", False, True, 0.25), (2, 67, 131, "soft", True, True, ALPHA_CUT), (2, 129, 257, "noise", False, False, MIN_CUT),
            (1, 200, 300, "disc80", False, False, ALPHA_CUT), (2, 32, 32, "const1", False, False, 1.0), (2, 40, 33, "hard", False, True, 1.0),
            (2, 96, 132, "dirty", True, True, 0.25), (2, 64, 128, "noise", False, True, ALPHA_CUT)]


@functools.lru_cache(maxsize=None)
def cases():
    """((name, image, alpha, bg, hole, alpha_cut), ...)"""
    out = []
    for i, (B, H, W, pat, with_bg, with_hole, cut) in enumerate(_case_specs()):
        name = f"{i:02d}_{pat}_{B}x{H}x{W}_cut{cut:g}{'_bg' if with_bg else ''}{'_hole' if with_hole else ''}"
        out.append((name, *inputs(pat, 11 * i, B, H, W, with_bg, with_hole), cut))
    return tuple(out)


def case_launches():
    """the launch counts of one run over the whole case list"""
    total = {}
    for _, image, *_ in cases():
        for k, v in launches(*image.shape[1:3]).items():
            total[k] = total.get(k, 0) + v
    return total


def references_for(image, alpha, bg, hole, alpha_cut):
    """(reference in fp64, d32)"""
    r64 = reference(image, alpha, bg, hole, alpha_cut, np.float64)
    d32 = float(np.abs(reference(image, alpha, bg, hole, alpha_cut, np.float32) - r64).max())
    return r64, d32


@functools.lru_cache(maxsize=None)
def _references(name):
    """Computed once per process and shared by every test that needs it."""
    _, image, alpha, bg, hole, cut = next(c for c in cases() if c[0] == name)
    return references_for(image, alpha, bg, hole, cut)


def tolerance(d32):
    return max(4.0 * d32, 2.0 ** -20)


def compare(name, out, refs, report=None):
    """out (a torch tensor on any device) against the references of a case, under the rule above."""
    r64, d32 = refs
    tol = tolerance(d32)
    out = out.detach().cpu()
    assert out.dtype == torch.float32 and tuple(out.shape) == r64.shape, (name, out.dtype, tuple(out.shape))
    out = out.numpy()
    assert np.isfinite(out).all(), name
    d = float(np.abs(out.astype(np.float64) - r64).max())
    line = f"[plate] {name}: d32 = {d32:.3e} tol = {tol:.3e} d = {d:.3e} ratio = {d / max(d32, 1e-30):.2f}"
    print(line)
    if report is not None:
        report.append(line)
    assert d <= tol, line


def _opt(to_tensor, t):
    return None if t is None else to_tensor(torch.from_numpy(t))


def check(fill, to_tensor, report=None):
    """fill(image, alpha, bg, hole, alpha_cut) -> out on tensors made by `to_tensor` from CPU tensors; every case."""
    for name, image, alpha, bg, hole, cut in cases():
        out = fill(_opt(to_tensor, image), _opt(to_tensor, alpha), _opt(to_tensor, bg), _opt(to_tensor, hole), cut)
        compare(name, out, _references(name), report)


def offset_copy(t):
    """A contiguous copy of the CPU tensor t that starts 4 bytes off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype)
    k = 1 + (-(buf.data_ptr() // 4) % 4)              # element k is 16-byte aligned + 4 bytes
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---- the identities of the header ---------------------------------------------------------------------------------------------------------
IDENTITY_SIZES = ((67, 131), (40, 72), (20, 24))      # tiled with seams; tiled, W % 4 == 0; one block


def check_identities(fill, to_tensor, H, W, who):
    """Identities 1 to 3 of include/sdmatte.h on tensors made by `to_tensor`, bit for bit."""
    image, alpha, bg, hole = inputs("dirty", 3, 2, H, W, with_bg=True, with_hole=True)
    t = lambda a: _opt(to_tensor, a)
    # 1. w_0 == 1 -> out == C, with and without bg / hole, at two cuts
    for b_, h_, cut in ((None, None, ALPHA_CUT), (bg, None, 1.0), (bg, hole, 0.25), (None, hole, MIN_CUT)):
        w0 = weights0(alpha, h_, cut)
        C = image if b_ is None else b_
        out = fill(t(image), t(alpha), t(b_), t(h_), cut).detach().cpu().numpy()
        keep = w0 == 1.0
        assert keep.any() and not keep.all(), (who, H, W)
        assert np.array_equal(out[keep], C[keep]), (who, H, W, cut)
        assert not np.array_equal(out, C), (who, H, W, cut)
    # 2. a channel that is 0 wherever w_0 > 0 is 0 in the whole plate, whatever it holds elsewhere
    w0 = weights0(alpha, hole, 0.25)
    dirty = image.copy()
    dirty[..., 1] = np.where(w0 > 0.0, 0.0, 0.9).astype(np.float32)
    assert (dirty[..., 1] > 0).any()
    out = fill(t(dirty), t(alpha), None, t(hole), 0.25).detach().cpu().numpy()
    assert np.all(out[..., 1] == 0.0) and np.any(out[..., 0] != 0.0), (who, H, W)
    # 3. a hard alpha and C == 0.5 wherever a == 0 -> exactly 0.5 everywhere
    hard = (sanitise(alpha) > 0.3).astype(np.float32)
    flat = np.where(hard[..., None] == 0.0, np.float32(0.5), image).astype(np.float32)
    for cut in (1.0, ALPHA_CUT):
        out = fill(t(flat), t(hard), None, None, cut).detach().cpu().numpy()
        assert np.all(out == 0.5), (who, H, W, cut, float(np.abs(out - 0.5).max()))


# ---- what the call is for ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def purpose_scene():
    """(image [1,200,300,3], alpha [1,200,300], true background [1,200,300,3]): a soft disc of colour (1, 0.1, 0.1) and radius 60 around (100, 150),
    composed over a background whose red is 0."""
    H, W = 200, 300
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    bgd = np.stack([np.zeros((H, W)), 0.2 + 0.6 * x / W + 0.05 * np.sin(x / 7.0) * np.cos(y / 9.0), 0.8 - 0.5 * y / H], -1)
    a = np.clip((60.0 - np.sqrt((y - 100.0) ** 2 + (x - 150.0) ** 2)) / 4.0 + 0.5, 0.0, 1.0)
    image = a[..., None] * np.array([1.0, 0.1, 0.1]) + (1.0 - a[..., None]) * bgd
    return image[None].astype(np.float32), a[None].astype(np.float32), bgd[None].astype(np.float32)


def _hole_errors(plate, truth, hole):
    """(max, mean) of |plate - truth| in g and b over the hole"""
    d = np.abs(np.asarray(plate, np.float64) - truth)[..., 1:][hole]
    return float(d.max()), float(d.mean())


@functools.lru_cache(maxsize=None)
def purpose_reference():
    """(reference(fp64) on the image alone at ALPHA_CUT, its d32, its (max, mean) error over the hole, the mean fill's (max, mean) error)"""
    image, alpha, truth = purpose_scene()
    r64, d32 = references_for(image, alpha, None, None, ALPHA_CUT)
    w0 = weights0(alpha, None, ALPHA_CUT).astype(np.float64)
    hole = w0 < 1.0
    mean = (w0[..., None] * image).sum((1, 2)) / w0.sum()
    filled = np.where(hole[..., None], mean[:, None, None, :], image.astype(np.float64))
    return r64, d32, _hole_errors(r64, truth, hole), _hole_errors(filled, truth, hole)


def check_purpose(fill, to_tensor, who):
    """The subject's red reaches no pixel of the plate - with the image alone and a hard alpha, and with a soft alpha and a bg plane that carries the
    subject's red wherever a >= alpha_cut (so it is not read through) - and the fill is close to the true background: no worse than reference(fp64) by
    more than the tolerance, which itself has at most half the error of filling with the weighted mean colour."""
    image, alpha, truth = purpose_scene()
    t = lambda a: _opt(to_tensor, a)
    hard = (alpha > 0.0).astype(np.float32)
    out = fill(t(image), t(hard), None, None, ALPHA_CUT).detach().cpu().numpy()
    assert np.all(out[..., 0] == 0.0), (who, float(out[..., 0].max()))
    bg_in = np.where((alpha >= np.float32(ALPHA_CUT))[..., None], image, truth).astype(np.float32)
    assert bg_in[..., 0].max() > 0.9
    out = fill(t(image), t(alpha), t(bg_in), None, ALPHA_CUT).detach().cpu().numpy()
    assert np.all(out[..., 0] == 0.0), (who, float(out[..., 0].max()))
    r64, d32, ref_err, mean_err = purpose_reference()
    tol = tolerance(d32)
    hole = weights0(alpha, None, ALPHA_CUT) < 1.0
    out = fill(t(image), t(alpha), None, None, ALPHA_CUT).detach().cpu().numpy()
    err = _hole_errors(out, truth, hole)
    line = (f"[plate] purpose ({who}): error over the hole max {err[0]:.4f} mean {err[1]:.4f}; reference(fp64) max {ref_err[0]:.4f} mean {ref_err[1]:.4f}; "
            f"mean fill max {mean_err[0]:.4f} mean {mean_err[1]:.4f}; red left in the hole {float(out[..., 0][hole].max()):.3f}; tol {tol:.3e}")
    print(line)
    assert ref_err[0] <= 0.5 * mean_err[0] and ref_err[1] <= 0.5 * mean_err[1], line
    assert err[0] <= ref_err[0] + tol and err[1] <= ref_err[1] + tol, line
    return line
