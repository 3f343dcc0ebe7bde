"""Shared by tests/test_node_defocus_cpu.py, tests/test_emu_defocus.py and tests/test_gpu_defocus.py: the background-defocus cases, the purpose scenes, and
a numpy reference of the function defined in include/sdmatte.h (sdm_defocus_background) that shares no code with the kernels (csrc/k_defocus.h) or with
the torch restatement (sdmatte_nodes.defocus_background).  The reference is callable in fp64 and fp32, in two variants:
  variant 0  sums each disc directly: one shifted add per offset (dy, dx) with dy^2 + dx^2 <= R^2, row-major;
  variant 1  takes inclusive prefix sums over each whole row, a disc row as the difference of two prefix values at x + hw(dy) and x - hw(dy) - 1 (clipped
             to the row), and sums the rows in descending dy.  hw(dy) is found in integers, by a search of its own.

Tolerance of `compare`, per case: max(4 * d32, 2**-20) on the max abs difference to reference(fp64).
  * d32 is the larger distance to reference(fp64) of the two fp32 variants.  It is computed here, never taken from the code under test.
  * Why this covers a prefix-sum kernel: variant 1 has the cancellation of a prefix scheme at whole-row magnitude (a kernel with segment-local prefixes is
    below it); variant 0 has the rounding of a long direct sum.
  * 4x: another fp32 evaluation differs in summation order, FMA contraction and division sequence, each a perturbation of the size of fp32 rounding (the
    margin of temporal_suite.py, guided_suite.py and foreground_suite.py).  `out` is well-conditioned even where N is tiny: 1 - a(p) <= N(p), so the
    factor 1 - a in front of Bb cancels what the small denominator amplifies.
  * floor 2**-20 = 8 ulp of 1.0, for constant inputs.
  * So that a disagreement of the two variants cannot hide in d32, `references_for` also asserts that they agree in fp64 (to 1e-9).
highlight_gain and highlight_threshold cross the C ABI as floats, so the reference rounds them the same way first: d32 measures arithmetic only.
reference(fp64) of a case is variant 0; the one larger GPU case (2 x 270 x 480, R = 32) takes variant 1 in fp64 (a prefix in fp64 is exact to 1e-12, and
variant 0 there costs seconds) and only its fp32 distance from variant 0."""
import functools

import numpy as np
import torch

FLOOR = 2.0 ** -10          # SDM_DEFOCUS_FLOOR


# ---- reference --------------------------------------------------------------------------------------------------------------------------
def sanitise_alpha(alpha):
    a = np.asarray(alpha, np.float32)
    a = np.where(np.isnan(a), np.float32(0), a)
    return np.minimum(np.maximum(a, np.float32(0)), np.float32(1)).astype(np.float32)


def half_widths(R):
    """hw[dy] for dy = 0 .. R: the largest h with h*h <= R*R - dy*dy, by counting up in integers"""
    out = []
    for dy in range(R + 1):
        h = 0
        while (h + 1) * (h + 1) + dy * dy <= R * R:
            h += 1
        out.append(h)
    return out


def disc_size(R):
    return sum(1 for dy in range(-R, R + 1) for dx in range(-R, R + 1) if dy * dy + dx * dx <= R * R)


def _disc_sums(planes, R, variant):
    """planes [B,H,W,4] -> the sums over the closed disc, pixels beyond the border absent"""
    B, H, W, _ = planes.shape
    acc = np.zeros_like(planes)
    if variant == 0:
        for dy in range(-R, R + 1):
            ya, yb = max(0, -dy), H - max(0, dy)
            if ya >= yb:
                continue
            for dx in range(-R, R + 1):
                if dy * dy + dx * dx > R * R:
                    continue
                xa, xb = max(0, -dx), W - max(0, dx)
                if xa < xb:
                    acc[:, ya:yb, xa:xb] += planes[:, ya + dy:yb + dy, xa + dx:xb + dx]
        return acc
    hw = half_widths(R)
    prefix = np.zeros((B, H, W + 1, 4), planes.dtype)          # prefix[..., x + 1, :] = sum of the row up to and including x
    np.cumsum(planes, axis=2, out=prefix[:, :, 1:])
    x = np.arange(W)
    for dy in range(R, -R - 1, -1):
        ya, yb = max(0, -dy), H - max(0, dy)
        if ya >= yb:
            continue
        h = hw[abs(dy)]
        hi, lo = np.minimum(x + h, W - 1) + 1, np.maximum(x - h - 1, -1) + 1
        acc[:, ya:yb] += prefix[:, ya + dy:yb + dy][:, :, hi] - prefix[:, ya + dy:yb + dy][:, :, lo]
    return acc


def reference(image, alpha, fg, bg, radius_px, highlight_gain, highlight_threshold, dtype=np.float64, variant=0):
    """image [B,H,W,3], alpha [B,H,W], fg / bg [B,H,W,3] or None -> out [B,H,W,3] in `dtype`"""
    one, zero = dtype(1), dtype(0)
    gain, thr, e = dtype(np.float32(highlight_gain)), dtype(np.float32(highlight_threshold)), dtype(FLOOR)
    img = np.asarray(image, np.float32).astype(dtype)
    a = sanitise_alpha(alpha).astype(dtype)
    C = img if bg is None else np.asarray(bg, np.float32).astype(dtype)
    F = img if fg is None else np.asarray(fg, np.float32).astype(dtype)
    Y = (C[..., 0] + C[..., 1] + C[..., 2]) / dtype(3)
    w = (one - a) * (one + gain * np.maximum(zero, Y - thr))
    planes = np.concatenate([w[..., None] * C, w[..., None]], -1)
    sums = _disc_sums(planes, int(radius_px), variant)
    blur = (sums[..., :3] + e * C) / (sums[..., 3:] + e)
    out = a[..., None] * F + (one - a[..., None]) * blur
    assert out.dtype == dtype
    return out


def naive_blur_then_lerp(image, alpha, radius_px):
    """What users do today: blur the photo with the same disc (normalised by the disc's pixels that exist), then mix by alpha."""
    img = np.asarray(image, np.float64)
    a = sanitise_alpha(alpha).astype(np.float64)[..., None]
    planes = np.concatenate([img, np.ones(img.shape[:3] + (1, ))], -1)
    sums = _disc_sums(planes, int(radius_px), 1)
    return a * img + (1.0 - a) * sums[..., :3] / sums[..., 3:]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
PATTERNS = ["soft", "hard", "const0", "const1", "noise", "dirty"]


def _texture(rng, B, H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for b in range(B):
        ph = rng.uniform(0.0, 6.0, 3)
        base = np.stack([0.5 + 0.3 * np.sin(x / 5.0 + ph[0]) * np.cos(y / 7.0), 0.5 + 0.3 * np.sin(y / 4.0 + ph[1]), 0.5 + 0.3 * np.cos((x + y) / 6.0 + ph[2])], -1)
        out.append(np.clip(base + rng.uniform(-0.2, 0.2, (H, W, 3)), 0.0, 1.0))
    return np.stack(out)


def inputs(pattern, seed, B, H, W, planes=False):
    """(image, alpha, fg or None, bg or None): images in [0, 1], different content per image of the batch."""
    rng = np.random.default_rng(seed + 5000)
    image = _texture(rng, B, H, W)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    alpha = np.zeros((B, H, W))
    for b in range(B):
        cy, cx = (0.45 + 0.1 * b) * H, (0.55 - 0.1 * b) * W
        d = np.sqrt((y - cy) ** 2 + (x - cx) ** 2)
        if pattern in ("soft", "dirty"):
            alpha[b] = np.clip(0.5 - (d - 0.3 * min(H, W)) / 3.0, 0.0, 1.0)
        elif pattern == "hard":          # larger than any disc of the list that fits the image: N -> 0 inside
            alpha[b] = (d <= 0.45 * max(H, W)).astype(np.float64)
        elif pattern == "const1":
            alpha[b] = 1.0
        elif pattern == "noise":
            alpha[b] = rng.uniform(size=(H, W))
    if pattern == "dirty":               # NaN and values outside [0, 1] sprinkled in
        pick = rng.uniform(size=alpha.shape)
        alpha[pick < 0.03] = np.nan
        alpha[(pick >= 0.03) & (pick < 0.06)] = -0.5
        alpha[(pick >= 0.06) & (pick < 0.09)] = 1.5
    fg = bg = None
    if planes:
        fg, bg = _texture(rng, B, H, W), _texture(rng, B, H, W)
    c = lambda t: None if t is None else np.ascontiguousarray(t, np.float32)
    return c(image), c(alpha), c(fg), c(bg)


def _case_specs():
    """(B, H, W, R): every radius of the list; W below one, across one and across two 256-column segment boundaries; ragged tile heights (tiles are 64
    rows); W < R and H < R; W = 1 and H = 1; R = 64 once."""
    return [(2, 70, 150, 5), (2, 90, 300, 32), (2, 40, 517, 17), (2, 33, 70, 1), (2, 67, 260, 2), (2, 65, 257, 17), (1, 140, 270, 64), (2, 40, 3, 17),
            (2, 1, 70, 5), (2, 37, 1, 5), (1, 1, 1, 2), (2, 3, 40, 17), (2, 20, 256, 32), (2, 130, 64, 5)]


@functools.lru_cache(maxsize=None)
def cases():
    """((name, image, alpha, fg, bg, (radius_px, highlight_gain, highlight_threshold)), ...): the alpha patterns in turn, every second case with the two
    colour planes, gain 0 and 4 (threshold 0.5) alternating out of step with them."""
    out = []
    for i, (B, H, W, R) in enumerate(_case_specs()):
        pat = PATTERNS[i % len(PATTERNS)]
        planes, gain = i % 2 == 1, (0.0, 0.0, 4.0, 4.0)[i % 4]
        out.append((f"{i:02d}_{pat}_{B}x{H}x{W}_R{R}_g{gain:g}{'_fgbg' if planes else ''}", *inputs(pat, 7 * i, B, H, W, planes), (R, gain, 0.5)))
    return tuple(out)


def references_for(image, alpha, fg, bg, params, fast64=False):
    """(reference in fp64, d32)"""
    r64 = reference(image, alpha, fg, bg, *params, dtype=np.float64, variant=1 if fast64 else 0)
    if not fast64:
        assert float(np.abs(reference(image, alpha, fg, bg, *params, dtype=np.float64, variant=1) - r64).max()) <= 1e-9
    d32 = max(float(np.abs(reference(image, alpha, fg, bg, *params, dtype=np.float32, variant=v) - r64).max()) for v in (0, 1))
    return r64, d32


@functools.lru_cache(maxsize=None)
def _references(name):
    """Computed once per process and shared by every test that needs it."""
    _, image, alpha, fg, bg, params = next(c for c in cases() if c[0] == name)
    return references_for(image, alpha, fg, bg, params)


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
    line = f"[defocus] {name}: d32 = {d32:.3e} tol = {tol:.3e} d = {d:.3e} ratio = {d / max(d32, 1e-30):.2f}"
    print(line)
    if report is not None:
        report.append(line)
    assert d <= tol, line


def _opt(to_tensor, t):
    return None if t is None else to_tensor(torch.from_numpy(t))


def check(defocus, to_tensor, report=None):
    """defocus(image, alpha, fg, bg, radius_px, highlight_gain, highlight_threshold) -> out on tensors made by `to_tensor` from CPU tensors; every case."""
    for name, image, alpha, fg, bg, params in cases():
        out = defocus(_opt(to_tensor, image), _opt(to_tensor, alpha), _opt(to_tensor, fg), _opt(to_tensor, bg), *params)
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
PURPOSE_R = 12


@functools.lru_cache(maxsize=None)
def purpose_scene():
    """(image [1,96,128,3], alpha [1,96,128]): a hard red disc (1, 0, 0) of radius 20 over a background whose red channel is 0 and whose blue channel
    is textured."""
    H, W = 96, 128
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    rng = np.random.default_rng(99)
    bgd = np.stack([np.zeros((H, W)), 0.4 + 0.2 * np.sin(x / 6.0), np.clip(0.5 + 0.3 * np.sin(x / 3.0) * np.cos(y / 4.0) + rng.uniform(-0.15, 0.15, (H, W)), 0, 1)], -1)
    subject = ((y - 48.0) ** 2 + (x - 64.0) ** 2) <= 20.0 ** 2
    image = np.where(subject[..., None], np.array([1.0, 0.0, 0.0]), bgd)
    return image[None].astype(np.float32), subject[None].astype(np.float32)


def _ring():
    """the background pixels within PURPOSE_R of the subject"""
    y, x = np.mgrid[0:96, 0:128].astype(np.float64)
    d = np.sqrt((y - 48.0) ** 2 + (x - 64.0) ** 2)
    return (d > 20.0) & (d <= 20.0 + PURPOSE_R)


def check_purpose(out, who):
    """out = the call on purpose_scene() at R = PURPOSE_R, gain 0.  The red of out is exactly 0 wherever a = 0 (no halo) while the blue of the ring
    around the subject did change (it blurred); the naive blur-then-lerp on the same scene puts a mean red above 0.1 into that ring."""
    image, alpha = purpose_scene()
    out = np.asarray(out, np.float32).reshape(image.shape)
    ring = _ring()
    red = out[0, ..., 0][alpha[0] == 0.0]
    blue = float(np.abs(out[0, ..., 2] - image[0, ..., 2])[ring].mean())
    naive = naive_blur_then_lerp(image, alpha, PURPOSE_R)[0, ..., 0][ring]
    line = (f"[defocus] purpose ({who}): red where a = 0: max {float(np.abs(red).max()):.3e}; blue changed by {blue:.3f} in the ring; naive blur: red "
            f"mean {float(naive.mean()):.3f} max {float(naive.max()):.3f} in the ring")
    print(line)
    assert float(naive.mean()) > 0.1, line
    assert np.all(red == 0.0), line
    assert blue > 0.02, line
    return line


SHAPE_RADII = (1, 2, 5, 17)


def shape_scene(R):
    """(image, alpha, (cy, cx)): one white pixel far from the border on black, alpha 0 everywhere."""
    H, W, cy, cx = 2 * R + 9, 2 * R + 12, R + 4, R + 6
    image = np.zeros((1, H, W, 3), np.float32)
    image[0, cy, cx] = 1.0
    return image, np.zeros((1, H, W), np.float32), (cy, cx)


def check_disc_shape(defocus, to_tensor, who):
    """With alpha 0 and gain 0 every weight is 1: out(p) = 1 / (n + e) on the closed disc around the white pixel (n = the disc's pixel count) and 0
    elsewhere, so out(p) > 1 / (2 n) exactly on dy^2 + dx^2 <= R^2.  Pins the membership rule and every hw off-by-one."""
    for R in SHAPE_RADII:
        image, alpha, (cy, cx) = shape_scene(R)
        out = defocus(to_tensor(torch.from_numpy(image)), to_tensor(torch.from_numpy(alpha)), None, None, R, 0.0, 0.5).detach().cpu().numpy()
        y, x = np.mgrid[0:image.shape[1], 0:image.shape[2]]
        want = ((y - cy) ** 2 + (x - cx) ** 2) <= R * R
        for c in range(3):
            got = out[0, ..., c] > 1.0 / (2 * disc_size(R))
            assert np.array_equal(got, want), (who, R, c, int((got != want).sum()))
