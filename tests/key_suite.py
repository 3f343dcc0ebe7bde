"""Shared by tests/test_node_key_cpu.py, tests/test_emu_key.py and tests/test_gpu_key.py: the green-screen cases, the purpose scene, and a numpy
reference of the two functions defined in include/sdmatte.h (sdm_screen_colour, sdm_chroma_key) that shares no code with the kernels (csrc/k_key.h) or
with the torch restatement (sdmatte_nodes.screen_colour / chroma_key).  The trimap inside it is `trimap_suite.separable`, the numpy reference of
sdm_make_trimap; the plate of the two-pass key is `plate_suite.reference`.

Comparison rules.
  * info (the histogram facts), key, trimap and despilled: equal BIT FOR BIT to the fp32 reference (compares, one rounding per operation, integers).
  * the screen colour: max abs difference to reference(fp64) within max(4 * d32, 2**-20).  d32 is the larger distance of two fp32 evaluations of the
    reference to fp64 (sequential sums over runs of 4096 pixels; one np.sum per image row), computed here, never taken from the code under test.  A mean
    of n values in [0, 1] summed in fp32 is off by a few 2**-24 times the depth of the summation; 4x because another fp32 evaluation differs in the
    tree, each a perturbation of that size; the floor 2**-20 = 8 ulp of 1.0 is for constant inputs (the margin and floor of harmonize_suite.py).
    Where reference(fp64) is not finite (a `dirty` image may select an infinite pixel) the result must be non-finite in the same way.

Inputs are multiples of 2**-10 (or NaN / infinite in `dirty`), so no subnormal decides a bit.  Case sizes: 1x1x1 and 1x3x5 (smallest), 2x9x37 (less than
one run, ragged), 3x67x130 (8710 pixels: three runs, scalar loads), 2x64x256 (vector loads, exactly one histogram block), 1x130x260 (three histogram
blocks, the last one ragged).

The purpose scene (200 x 300: a screen lit 0.55 to 1.0 from left to right with noise of sigma 0.01, a disc with a 12-pixel soft edge that carries grey,
white and black patches and green spill), measured with the reference at erode = dilate = 16: no definite pixel of the trimap is wrong (definite
foreground has true alpha >= 0.9, definite background <= 0.1); the figures of the one-pass and the two-pass key are printed by `check_purpose`."""
import functools

import numpy as np
import torch

import plate_suite
import trimap_suite

MIN_SUM, MIN_SAT, MIN_SEP, RUN = np.float32(0.15), np.float32(0.25), np.float32(1.0 / 64), 4096      # SDM_KEY_*
DEFAULTS = (0.15, 0.85, 0.05, 0.95, 10, 10, 1.0)      # clip_fg, clip_bg, sure_fg, sure_bg, erode_px, dilate_px, despill
OUTPUTS = ("key", "trimap", "despilled")
COLOUR_LAUNCHES = ("ck_clear", "ck_hist", "ck_mode", "ck_mean", "ck_finalize")
HINT_NAMES = {0: "any", 1: "green", 2: "blue"}


# ---- reference: the screen colour ---------------------------------------------------------------------------------------------------------
def eligible_bins(image, hint):
    """(eligible bool, bin index int64) per pixel, in fp32"""
    c = np.asarray(image, np.float32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    with np.errstate(all="ignore"):
        s = (r + g) + b
        mx, mn = r.copy(), r.copy()
        for ch in (g, b):
            up, down = ch > mx, ch < mn
            mx[up], mn[down] = ch[up], ch[down]
        ok = (s >= MIN_SUM) & ((mx - mn) >= MIN_SAT * s)
        if hint == 1:
            ok &= (g > r) & (g > b)
        if hint == 2:
            ok &= (b > r) & (b > g)
        idx = []
        for ch in (r, g):
            u = (ch / s) * np.float32(64)
            assert u.dtype == np.float32
            i = np.zeros(u.shape, np.int64)
            inside = (u >= 0) & (u < 64)
            i[inside] = np.trunc(u[inside]).astype(np.int64)
            i[u >= 64] = 63
            idx.append(i)
    return ok, idx[0] * 64 + idx[1]


def _mode(hist):
    best, arg = -1, 0
    for iu in range(64):
        for iv in range(64):
            c = int(hist[max(iu - 1, 0):iu + 2, max(iv - 1, 0):iv + 2].sum())
            if c > best:
                best, arg = c, iu * 64 + iv
    return arg


def _mean(vals, n, W, variant):
    """vals: the slot's pixels [P,3] with the unselected ones zeroed"""
    if variant == "f64":
        return vals.astype(np.float64).sum(axis=0) / n
    step = RUN if variant == "runs32" else W
    tot = np.zeros(3, np.float64)
    with np.errstate(all="ignore"):
        for p0 in range(0, vals.shape[0], step):
            part = vals[p0:p0 + step].astype(np.float32)
            tot += (np.cumsum(part, axis=0, dtype=np.float32)[-1] if variant == "runs32" else part.sum(axis=0, dtype=np.float32)).astype(np.float64)
        return tot / n


def colour_reference(image, hint, share, variant="f64"):
    """-> (colour float64 [B,3] (the fp32 variants rounded to fp32 and widened), info int32 [B,4])"""
    image = np.asarray(image, np.float32)
    B, H, W, _ = image.shape
    ok, idx = eligible_bins(image, hint)
    slots = 1 if share else B
    ok, idx, px = ok.reshape(slots, -1), idx.reshape(slots, -1), image.reshape(slots, -1, 3)
    colour, info = np.zeros((slots, 3), np.float64), np.zeros((slots, 4), np.int32)
    for s in range(slots):
        if not ok[s].any():
            info[s] = (0, 0, -1, -1)
            continue
        hist = np.zeros(4096, np.int64)
        np.add.at(hist, idx[s][ok[s]], 1)
        mode = _mode(hist.reshape(64, 64))
        mu, mv = divmod(mode, 64)
        sel = ok[s] & (np.abs(idx[s] // 64 - mu) <= 1) & (np.abs(idx[s] % 64 - mv) <= 1)
        n = int(sel.sum())
        with np.errstate(all="ignore"):
            m = _mean(np.where(sel[:, None], px[s], np.float32(0)), n, W, variant)
            colour[s] = m if variant == "f64" else m.astype(np.float32).astype(np.float64)
        info[s] = (int(ok[s].sum()), n, mu, mv)
    rep = B if share else 1
    return np.repeat(colour, rep, axis=0), np.repeat(info, rep, axis=0)


# ---- reference: the key -------------------------------------------------------------------------------------------------------------------
def key_reference(image, screen, params=DEFAULTS, dtype=np.float32):
    """image [B,H,W,3], screen [B,3] or [B,H,W,3] -> {"key", "trimap", "despilled", "cls"} (cls: 1 F, 0 B, 2 U) in `dtype`; the inputs and the
    parameters are fp32 values in either case."""
    cf, cb, sf, sb, erode_px, dilate_px, ds = params
    cf, cb, sf, sb, ds = (dtype(np.float32(v)) for v in (cf, cb, sf, sb, ds))
    c = np.asarray(image, np.float32).astype(dtype)
    B, H, W, _ = c.shape
    S = np.asarray(screen, np.float32).astype(dtype)
    S = np.broadcast_to(S.reshape(B, 1, 1, 3) if S.ndim == 2 else S, c.shape)
    with np.errstate(all="ignore"):
        k = np.zeros((B, H, W), np.int64)
        k[S[..., 1] > S[..., 0]] = 1
        Sk = np.take_along_axis(S, k[..., None], -1)[..., 0]
        k[S[..., 2] > Sk] = 2
        o1, o2 = np.where(k == 0, 1, 0), np.where(k == 2, 1, 2)
        pick = lambda v, i: np.take_along_axis(v, i[..., None], -1)[..., 0]

        def y(v):
            a, b = pick(v, o1), pick(v, o2)
            return np.where(a > b, a, b)
        ck = pick(c, k)
        m, mS = ck - y(c), pick(S, k) - y(S)
        valid = (mS >= dtype(MIN_SEP)) & np.isfinite(m)
        q = (cb * mS - m) / ((cb - cf) * mS)
        assert q.dtype == dtype
        key = np.ones((B, H, W), dtype)
        key[valid & ~(q > 0)] = 0
        mid = valid & (q > 0) & (q < 1)
        key[mid] = q[mid]
        cls = np.full((B, H, W), 2, np.uint8)
        is_f = valid & (m <= sf * mS)
        cls[is_f] = 1
        cls[valid & ~is_f & (m >= sb * mS)] = 0
        t0 = trimap_suite.separable(key.astype(np.float32), 0.5, int(erode_px), int(dilate_px))
        keep = ((t0 == 1) & (cls == 1)) | ((t0 == 0) & (cls == 0)) | (t0 == 0.5)
        trimap = np.where(keep, t0, np.float32(0.5)).astype(dtype)
        desp = c.copy()
        spill = valid & (m > 0)
        d = ck - ds * m
        for ch in range(3):
            w = spill & (k == ch)
            desp[..., ch][w] = d[w]
    return {"key": key, "trimap": trimap, "despilled": desp, "cls": cls}


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
KINDS = ("screen", "blue", "noise", "flat", "grey", "dirty")


def _quantise(a):
    return (np.round(np.asarray(a, np.float64) * 1024) / 1024).astype(np.float32)


def _screen_scene(rng, B, H, W, colour):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    light = 0.55 + 0.45 * x / max(W - 1, 1)
    out = np.zeros((B, H, W, 3))
    for b in range(B):
        scr = light[..., None] * np.asarray(colour) + rng.normal(0, 0.01, (H, W, 3))
        cy, cx, rad = H * (0.4 + 0.1 * b), W * (0.45 + 0.05 * b), 0.3 * min(H, W) + 1
        a = np.clip((rad - np.hypot(y - cy, x - cx)) / max(0.2 * rad, 1.0) + 0.5, 0, 1)[..., None]
        fg = 0.2 + 0.6 * rng.random((1, 1, 3)) + rng.normal(0, 0.05, (H, W, 3))
        out[b] = a * fg + (1 - a) * scr
    return np.clip(out, 0, 1)


def inputs(kind, seed, B, H, W):
    """image fp32 [B,H,W,3]: 0 or at least 2**-10 in magnitude (multiples of 2**-10), `dirty` also NaN and the infinities"""
    rng = np.random.default_rng(1000 + seed)
    if kind in ("screen", "dirty"):
        img = _screen_scene(rng, B, H, W, (0.10, 0.75, 0.20))
    elif kind == "blue":
        img = _screen_scene(rng, B, H, W, (0.10, 0.25, 0.80))
    elif kind == "noise":
        img = rng.random((B, H, W, 3))
    elif kind == "flat":
        img = np.ones((B, H, W, 3)) * np.array([0.125, 0.75, 0.25])
    elif kind == "grey":
        img = np.repeat(rng.random((B, H, W, 1)), 3, axis=-1)
    else:
        raise ValueError(kind)
    img = _quantise(img)
    if kind == "dirty":
        flat = img.reshape(-1)
        n = flat.size
        for v in (np.nan, np.inf, -np.inf, -0.5, -2.0 ** -10, 1.5, 4.0, 0.0):
            flat[rng.choice(n, max(1, n // 40), replace=False)] = v
    return img


def offset_copy(t):
    """A contiguous copy of the CPU tensor t that starts 4 bytes off a 16-byte boundary."""
    return _harmonize_suite().offset_copy(t)


def _harmonize_suite():
    import harmonize_suite
    return harmonize_suite


# ---- the case list ------------------------------------------------------------------------------------------------------------------------
# (name, kind, B, H, W, hint, share)
CASES = (("flat_1x1x1_green", "flat", 1, 1, 1, 1, 0),
         ("screen_1x3x5_any", "screen", 1, 3, 5, 0, 0),
         ("grey_1x3x5_green", "grey", 1, 3, 5, 1, 0),
         ("blue_2x9x37_blue_share", "blue", 2, 9, 37, 2, 1),
         ("dirty_3x67x130_green", "dirty", 3, 67, 130, 1, 0),
         ("screen_3x67x130_any_share", "screen", 3, 67, 130, 0, 1),
         ("flat_2x64x256_green", "flat", 2, 64, 256, 1, 0),
         ("noise_2x64x256_any_share", "noise", 2, 64, 256, 0, 1),
         ("screen_1x130x260_green", "screen", 1, 130, 260, 1, 0),
         ("noise_1x130x260_blue", "noise", 1, 130, 260, 2, 0))
RADII = ((0, 0), (1, 3), (10, 10))
BIG_RADIUS_CASE = ("screen_1x40x70_green", "screen", 1, 40, 70, 1, 0)
# per radii: the outputs asked for (every output alone and all together, over the three)
WANTS = {(0, 0): (("key", ), ("trimap", ), ("despilled", )), (1, 3): (("trimap", "key"), ), (10, 10): (OUTPUTS, ), (255, 255): (("trimap", ), )}


@functools.lru_cache(maxsize=None)
def case_image(name):
    _, kind, B, H, W, _, _ = next(c for c in CASES + (BIG_RADIUS_CASE, ) if c[0] == name)
    img = inputs(kind, len(name), B, H, W)
    img.setflags(write=False)
    return img


def tolerance(d32):
    return max(4.0 * d32, 2.0 ** -20)


@functools.lru_cache(maxsize=None)
def colour_refs(name):
    """(colour64 [B,3], info [B,4], d32): computed once per process and shared by every test that needs it"""
    _, _, _, _, _, hint, share = next(c for c in CASES + (BIG_RADIUS_CASE, ) if c[0] == name)
    c64, info = colour_reference(case_image(name), hint, share, "f64")
    d32 = 0.0
    for variant in ("runs32", "rows32"):
        c32, i32 = colour_reference(case_image(name), hint, share, variant)
        assert np.array_equal(i32, info)
        fin = np.isfinite(c64)
        assert np.array_equal(np.isfinite(c32), fin)
        if fin.any():
            d32 = max(d32, float(np.abs(c32 - c64)[fin].max()))
    return c64, info, d32


def compare_colour(name, colour, info, refs):
    c64, i_ref, d32 = refs
    colour, info = colour.detach().cpu(), info.detach().cpu()
    assert colour.dtype == torch.float32 and tuple(colour.shape) == c64.shape and info.dtype == torch.int32, (name, colour.dtype, tuple(colour.shape))
    assert np.array_equal(info.numpy(), i_ref), (name, info.numpy(), i_ref)
    got = colour.numpy().astype(np.float64)
    fin = np.isfinite(c64)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(np.isnan(got), np.isnan(c64)), (name, got, c64)
    diff = float(np.abs(got - c64)[fin].max()) if fin.any() else 0.0
    line = f"[key] {name} colour: d32 = {d32:.3e} tol = {tolerance(d32):.3e} d = {diff:.3e}"
    print(line)
    assert diff <= tolerance(d32), line


def check_colour(screen_colour, to_tensor):
    """screen_colour(image, hint, share, return_info=True) -> (colour, info) on tensors made by `to_tensor` from CPU tensors; every case."""
    for name, _, _, _, _, hint, share in CASES:
        colour, info = screen_colour(to_tensor(torch.from_numpy(case_image(name).copy())), HINT_NAMES[hint], bool(share), return_info=True)
        compare_colour(name, colour, info, colour_refs(name))
    return len(CASES)


def bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def case_screens(name):
    """The two screen forms a case is keyed against: the reference's own colour (rounded to fp32), and a plane that varies per pixel."""
    img = case_image(name)
    B, H, W, _ = img.shape
    colour = np.nan_to_num(colour_refs(name)[0], nan=0.5, posinf=1.0, neginf=0.0).astype(np.float32)
    if not colour.any():
        colour = np.tile(np.float32([0.125, 0.75, 0.25]), (B, 1))      # (a case without eligible pixels is keyed against a green of its own)
    x = np.linspace(0.5, 1.0, W, dtype=np.float64)[None, None, :, None]
    plane = _quantise(colour.astype(np.float64)[:, None, None, :] * x * np.ones((B, H, W, 3)))
    return colour, plane


@functools.lru_cache(maxsize=None)
def key_refs(name, plane, radii):
    colour, pl = case_screens(name)
    return key_reference(case_image(name), pl if plane else colour, DEFAULTS[:4] + tuple(radii) + (1.0, ))


def key_plan(big_radius=True):
    """[(case name, plane?, radii, want)]: every case with both screen forms, the three radii pairs and every output alone and together"""
    plan = []
    for i, (name, *_) in enumerate(CASES):
        for radii in RADII:
            for j, want in enumerate(WANTS[radii]):
                plan.append((name, (i + j + radii[0]) % 2 == 1, radii, want))
        plan.append((name, i % 2 == 0, (10, 10), ("key", "despilled")))
    if big_radius:
        plan.append((BIG_RADIUS_CASE[0], False, (255, 255), ("trimap", )))
    return plan


def key_launches(plan):
    out = {}
    for _, _, _, want in plan:
        for k in (("ck_key", "trimap_cols", "trimap_rows", "ck_veto") if "trimap" in want else ("ck_key", )):
            out[k] = out.get(k, 0) + 1
    return out


def check_key(chroma_key, to_tensor, big_radius=True):
    """chroma_key(image, screen, clip_fg, clip_bg, sure_fg, sure_bg, erode_px, dilate_px, despill, want=...) on tensors made by `to_tensor` from CPU
    tensors; every entry of the plan, bit for bit.  Returns the plan."""
    plan = key_plan(big_radius)
    assert {p[1] for p in plan} == {False, True} and {w for p in plan for w in p[3]} == set(OUTPUTS)
    for name, plane, radii, want in plan:
        colour, pl = case_screens(name)
        ref = key_refs(name, plane, radii)
        got = chroma_key(to_tensor(torch.from_numpy(case_image(name).copy())), to_tensor(torch.from_numpy(pl if plane else colour)), *DEFAULTS[:4], *radii, 1.0,
                         want=want)
        got = got if isinstance(got, tuple) else (got, )
        assert len(got) == len(want)
        for w, g in zip(want, got):
            assert g.dtype == torch.float32 and tuple(g.shape) == ref[w].shape, (name, w, g.dtype, tuple(g.shape))
            bad = int((bits(g) != bits(ref[w])).sum())
            assert bad == 0, f"[key] {name} plane={plane} radii={radii} want={want}: {w} differs from the fp32 reference in {bad} values"
    return plan


# ---- identities ---------------------------------------------------------------------------------------------------------------------------
def check_identities(screen_colour, chroma_key, to_tensor, who, H=67, W=130):
    """The seven identities of include/sdmatte.h, bit for bit (6 without its pointer-kind and alignment parts, which belong to the engine's tests)."""
    T = lambda a: to_tensor(torch.from_numpy(np.ascontiguousarray(a)))
    img = inputs("dirty", 11, 3, H, W)
    colour = np.float32([[0.125, 0.75, 0.25], [0.25, 0.25, 0.75], [0.5, 0.5, 0.5]])
    # 1. despill = 0 copies the image
    d0 = chroma_key(T(img), T(colour), *DEFAULTS[:6], 0.0, want=("despilled", ))
    assert same_bits(d0, img), (who, 1)
    # 2. a valid pixel equal to its screen colour has key 0 and class B; 3. a valid pixel with r = g = b has key 1 and class F (the class is read off
    # the trimap at radii 0: T0 is then the key's own side of 0.5, and the veto leaves 0.5 where the class disagrees)
    rng = np.random.default_rng(5)
    plane = _quantise(0.1 + 0.8 * rng.random((3, H, W, 3)))
    valid = key_reference(plane, plane)["cls"] != 2
    assert valid.any() and not valid.all()
    key, tri = chroma_key(T(plane), T(plane), *DEFAULTS[:4], 0, 0, 1.0, want=("key", "trimap"))
    key, tri = key.detach().cpu().numpy(), tri.detach().cpu().numpy()
    assert (key[valid] == 0).all() and (tri[valid] == 0).all() and (key[~valid] == 1).all() and (tri[~valid] == 0.5).all(), (who, 2)
    grey = np.repeat(_quantise(rng.random((3, H, W, 1))), 3, axis=-1)
    key, tri, desp = chroma_key(T(grey), T(colour), *DEFAULTS[:4], 0, 0, 1.0, want=OUTPUTS)
    key, tri = key.detach().cpu().numpy(), tri.detach().cpu().numpy()
    assert (key == 1).all() and (tri[:2] == 1).all() and (tri[2] == 0.5).all() and same_bits(desp, grey), (who, 3)      # (image 2's screen is grey: invalid)
    # 4. a constant plane gives the bits of the colour form
    const = np.ascontiguousarray(np.broadcast_to(colour[:, None, None, :], img.shape))
    a = chroma_key(T(img), T(colour), *DEFAULTS[:4], 3, 5, 0.75, want=OUTPUTS)
    b = chroma_key(T(img), T(const), *DEFAULTS[:4], 3, 5, 0.75, want=OUTPUTS)
    assert all(same_bits(x, y) for x, y in zip(a, b)), (who, 4)
    # 6. batch against single images, and a second call
    b2 = chroma_key(T(img), T(colour), *DEFAULTS[:4], 3, 5, 0.75, want=OUTPUTS)
    assert all(same_bits(x, y) for x, y in zip(a, b2)), (who, 6)
    c_all, i_all = screen_colour(T(img), "any", False, return_info=True)
    for i in range(3):
        one = chroma_key(T(img[i:i + 1]), T(colour[i:i + 1]), *DEFAULTS[:4], 3, 5, 0.75, want=OUTPUTS)
        assert all(same_bits(x[i:i + 1], y) for x, y in zip(a, one)), (who, 6, i)
        c1, i1 = screen_colour(T(img[i:i + 1]), "any", False, return_info=True)
        assert same_bits(c_all[i:i + 1], c1) and torch.equal(i_all[i:i + 1].cpu(), i1.cpu()), (who, 6, i)
    # 7. share = 1 equals the call on the images laid end to end as one image of B * H rows
    clean = inputs("screen", 12, 3, H, W)
    for im in (clean, img):
        cs, is_ = screen_colour(T(im), "green", True, return_info=True)
        c1, i1 = screen_colour(T(im.reshape(1, 3 * H, W, 3)), "green", False, return_info=True)
        assert torch.equal(is_.cpu(), i1.cpu().expand(3, 4)) and all(same_bits(cs[i:i + 1], c1) for i in range(3)), (who, 7)
    # 5. the trimap equals the formula, evaluated on the call's own key: in `check_trimap_formula`, which needs a make_trimap


def check_trimap_formula(chroma_key, make_trimap, to_tensor, who, H=67, W=130):
    """Identity 5: the trimap is make_trimap(key, 0.5, erode_px, dilate_px), evaluated on the call's own key output, with the veto of the classes; the
    classes are those of the numpy reference (they are made of compares and products of the inputs alone, and `check_key` holds the code under test to
    them bit for bit)."""
    T = lambda a: to_tensor(torch.from_numpy(np.ascontiguousarray(a)))
    img = inputs("dirty", 13, 2, H, W)
    colour = np.float32([[0.125, 0.75, 0.25], [0.25, 0.25, 0.75]])
    for radii in ((2, 7), (10, 10)):
        key, tri = chroma_key(T(img), T(colour), *DEFAULTS[:4], *radii, 1.0, want=("key", "trimap"))
        t0 = make_trimap(key, 0.5, *radii).detach().cpu().numpy()
        cls = key_reference(img, colour)["cls"]
        keep = ((t0 == 1) & (cls == 1)) | ((t0 == 0) & (cls == 0)) | (t0 == 0.5)
        assert np.array_equal(tri.detach().cpu().numpy(), np.where(keep, t0, np.float32(0.5))), (who, 5, radii)


# ---- the purpose scene --------------------------------------------------------------------------------------------------------------------
PURPOSE_RADII = (16, 16)
PURPOSE_CUT = 0.25


@functools.lru_cache(maxsize=None)
def purpose_scene():
    """(image fp32 [1,200,300,3], true alpha float64 [1,200,300])"""
    H, W = 200, 300
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    light = (0.55 + 0.45 * x / (W - 1))[..., None]
    scr = light * np.array([0.10, 0.75, 0.20]) + rng.normal(0, 0.01, (H, W, 3))
    d = np.hypot(y - 100, x - 150)
    alpha = np.clip((66 - d) / 12, 0, 1)
    fg = np.full((H, W, 3), 0.5)
    fg[70:95, 120:150] = 0.95                                           # a white, a black and a mid-grey patch
    fg[105:130, 150:180] = 0.03
    fg[75:100, 160:185] = 0.3
    fg += rng.normal(0, 0.01, (H, W, 3))
    fg[..., 1] += 0.06 * np.clip((d - 30) / 36, 0, 1)                   # green spill towards the edge
    img = alpha[..., None] * fg + (1 - alpha[..., None]) * scr
    return _quantise(np.clip(img, 0, 1))[None], alpha[None]


def purpose_figures(trimap, key, alpha):
    trimap, key = np.asarray(trimap, np.float64), np.asarray(key, np.float64)
    fg_wrong = int(((trimap == 1) & (alpha < 0.9)).sum())
    bg_wrong = int(((trimap == 0) & (alpha > 0.1)).sum())
    return fg_wrong, bg_wrong, float((trimap == 0.5).mean()), float(np.abs(key - alpha).mean())


def _assert_purpose(who, one, two, desp):
    print(f"[key] purpose ({who}): one pass unknown {one[2]:.4f} key error {one[3]:.4f}; two passes unknown {two[2]:.4f} key error {two[3]:.4f}")
    assert one[0] == 0 and one[1] == 0 and two[0] == 0 and two[1] == 0, (who, one, two)
    assert two[2] < one[2] and two[3] < one[3], (who, one, two)
    desp = np.asarray(desp, np.float64)
    excess = float((desp[..., 1] - np.maximum(desp[..., 0], desp[..., 2])).max())      # (the screen is green: k = 1 everywhere)
    assert excess <= 2.0 ** -20, (who, excess)


@functools.lru_cache(maxsize=None)
def purpose_reference():
    """(one-pass figures, two-pass figures) of the reference; asserts the conditions on it"""
    img, alpha = purpose_scene()
    params = DEFAULTS[:4] + PURPOSE_RADII + (1.0, )
    colour = colour_reference(img, 1, 0)[0].astype(np.float32)
    r1 = key_reference(img, colour, params)
    plate = plate_suite.reference(img, r1["key"], None, None, PURPOSE_CUT, np.float32)
    r2 = key_reference(img, plate, params)
    assert (np.argmax(plate, axis=-1) == 1).all()
    one, two = purpose_figures(r1["trimap"], r1["key"], alpha), purpose_figures(r2["trimap"], r2["key"], alpha)
    _assert_purpose("reference", one, two, r2["despilled"])
    return one, two


def check_purpose(screen_colour, chroma_key, fill_background, to_tensor, who, key_screen=None):
    """The conditions on the reference first, then on the code under test; with `key_screen` also that the one call equals the chain bit for bit."""
    purpose_reference()
    img, alpha = purpose_scene()
    t = to_tensor(torch.from_numpy(img))
    colour = screen_colour(t, "green", False)
    args = DEFAULTS[:4] + PURPOSE_RADII + (1.0, )
    k1, t1, _ = chroma_key(t, colour, *args, want=OUTPUTS)
    plate = fill_background(t, k1, alpha_cut=PURPOSE_CUT)
    k2, t2, d2 = chroma_key(t, plate, *args, want=OUTPUTS)
    n = lambda v: v.detach().cpu().numpy()
    _assert_purpose(who, purpose_figures(n(t1), n(k1), alpha), purpose_figures(n(t2), n(k2), alpha), n(d2))
    if key_screen is not None:
        got = key_screen(t, "green", False, True, PURPOSE_CUT, *args, want=OUTPUTS)
        assert len(got) == 4 and all(same_bits(a, b) for a, b in zip(got, (k2, t2, d2, plate))), who
        got = key_screen(t, "green", False, False, PURPOSE_CUT, *args, want=("trimap", "key"))
        assert len(got) == 3 and same_bits(got[0], t1) and same_bits(got[1], k1) and same_bits(got[2], colour), who
