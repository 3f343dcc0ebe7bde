"""Shared by tests/test_emu_edge.py, tests/test_node_edge_cpu.py and tests/test_gpu_edge.py: the cases of the distance field (sdm_distance_field) and of its
two consumers (sdm_offset_mask, sdm_outline), with references that share no code with the kernels (csrc/k_distance.h):
  * `brute_force`: every pixel against every pixel of the other class, in int64 - the definition itself, for the sizes where N^2 is affordable;
  * the CPU restatement `sdmatte_nodes.distance_field` (column scans + an outward row search), proven equal to the brute force on every small case by
    tests/test_node_edge_cpu.py;
  * closed forms (a set of seed pixels, its complement, one seed in a long row) where the restatement is slow.
The field is integer arithmetic: every comparison of it is exact (np.array_equal).  The consumers go against the fp64 restatement under the rule of
guided_suite.tolerance: tol = max(4 * d32, 2^-20) with d32 the deviation of the fp32 restatement from the fp64 one on the same case."""
import functools

import numpy as np
import torch

import guided_suite as GS
import trimap_suite as TS

NONE = 2147483647
DF_KERNELS = {"field": ("df_bits", "df_carry", "df_cols", "df_rows"), "offset": ("df_bits", "df_carry", "df_cols", "df_offset"),
              "outline": ("df_bits", "df_carry", "df_cols", "df_outline")}


# ---- references -------------------------------------------------------------------------------------------------------------------------
def _foreground(plane, threshold):
    with np.errstate(invalid="ignore"):
        return np.asarray(plane, np.float32) > np.float32(threshold)      # one fp32 compare: NaN is outside F


def brute_force(plane, threshold):
    """int32 [B,H,W]: every pixel against every pixel of the other class of its image."""
    fg = _foreground(plane, threshold)
    B, H, W = fg.shape
    assert H * W <= 2048, "brute force is for small planes"
    ys, xs = np.divmod(np.arange(H * W, dtype=np.int64), W)
    d2 = (ys[:, None] - ys[None, :]) ** 2 + (xs[:, None] - xs[None, :]) ** 2
    out = np.empty((B, H, W), np.int32)
    for b in range(B):
        f = fg[b].reshape(-1)
        other = f[:, None] != f[None, :]
        best = np.where(other, d2, np.int64(NONE)).min(axis=1)
        out[b] = np.where(f, best, -best).reshape(H, W).astype(np.int32)
    return out


def seed_field(H, W, seeds):
    """Closed form for F = a set of seed pixels: int32 [H,W].  A background pixel's d2 is the minimum over the seeds; a seed's own d2 is found by looking
    at the pixels around it in rings of growing Chebyshev radius (1 for an isolated seed, more inside a clump)."""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
    best = np.full((H, W), np.int64(NONE))
    for y0, x0 in seeds:
        np.minimum(best, (ys - y0) ** 2 + (xs - x0) ** 2, out=best)
    out = -best
    sset = set(seeds)
    assert len(sset) < H * W
    for y0, x0 in sset:
        r, found = 0, None
        while found is None or r * r < found:      # a ring of radius r holds nothing nearer than r
            r += 1
            for y in range(max(0, y0 - r), min(H, y0 + r + 1)):
                for x in range(max(0, x0 - r), min(W, x0 + r + 1)):
                    if max(abs(y - y0), abs(x - x0)) == r and (y, x) not in sset:
                        d = (y - y0) ** 2 + (x - x0) ** 2
                        found = d if found is None else min(found, d)
        out[y0, x0] = found
    return out.astype(np.int32)


def seed_plane(H, W, seeds):
    p = np.zeros((H, W), np.float32)
    for y, x in seeds:
        p[y, x] = 1.0
    return p


def random_seeds(seed, H, W, k):
    """k seed pixels, among them a touching pair, a plus-shaped clump (its centre's nearest other pixel is a diagonal one: d2 = 2) and two corners."""
    rng = np.random.default_rng(seed)
    s = [(int(rng.integers(0, H)), int(rng.integers(0, W))) for _ in range(k - 9)]
    y, x = H // 3, W // 2
    return s + [(y, x), (y, x + 1), (2 * y, x), (2 * y - 1, x), (2 * y + 1, x), (2 * y, x - 1), (2 * y, x + 1), (0, 0), (H - 1, W - 1)]


@functools.lru_cache(maxsize=None)
def seed_case(H, W, k=50):
    """(plane fp32 [2,H,W], field int32 [2,H,W]): two different seed sets; the complement planes 1 - plane have the field -field."""
    sets = [random_seeds(H + b, H, W, k) for b in range(2)]
    return np.stack([seed_plane(H, W, s) for s in sets]), np.stack([seed_field(H, W, s) for s in sets])


def long_row_case(W=32768, x0=20000):
    plane = np.zeros((1, 1, W), np.float32)
    plane[0, 0, x0] = 1.0
    xs = np.arange(W, dtype=np.int64)
    field = -((xs - x0) ** 2)
    field[x0] = 1
    return plane, field.astype(np.int32).reshape(1, 1, W)


# ---- planes -----------------------------------------------------------------------------------------------------------------------------
BRUTE_SIZES = [(1, 1), (1, 9), (7, 1), (20, 33), (31, 45)]
# 130 x 257: rows longer than a 256-thread segment (five 64-column chunks); 8 x 2500 / 2500 x 8: one long envelope, one long column chain (79 tiles)
RESTATEMENT_SIZES = [(1, 1), (1, 70), (70, 1), (45, 70), (64, 64), (96, 128), (130, 257), (8, 2500), (2500, 8)]


def contents(H, W):
    """[(name, plane fp32 [H,W], threshold)] - the issue's list of contents at one size."""
    out = [("empty", np.zeros((H, W), np.float32), 0.5), ("full", np.ones((H, W), np.float32), 0.5)]
    corner = np.zeros((H, W), np.float32)
    corner[H - 1, W - 1] = 1.0
    out.append(("corner_pixel", corner, 0.5))
    ys, xs = np.mgrid[0:H, 0:W]
    out.append(("checkerboard", ((ys + xs) % 2).astype(np.float32), 0.5))
    half = np.zeros((H, W), np.float32)
    half[:, : (W + 1) // 2] = 1.0
    if W == 1:
        half[: H // 2] = 0.0
    out.append(("half_plane", half, 0.5))
    bl = TS.blobs(H * 1000 + W, 1, H, W)[0]
    out.append(("blobs", bl, 0.5))
    nan = bl.copy()
    nan[::3, ::5] = np.nan
    out.append(("nan", nan, 0.5))
    out.append(("soft_at_0.3", bl, 0.3))
    return out


@functools.lru_cache(maxsize=None)
def field_cases(kind):
    """[(name, plane fp32 [1,H,W], threshold, field int32 [1,H,W])] with the reference computed once: kind "brute" or "restatement"."""
    from comfyui_sdmatte_amd.sdmatte_nodes import distance_field
    out = []
    for H, W in (BRUTE_SIZES if kind == "brute" else RESTATEMENT_SIZES):
        for name, plane, thr in contents(H, W):
            plane = plane[None]
            want = brute_force(plane, thr) if kind == "brute" else distance_field(torch.from_numpy(plane), thr).numpy()
            out.append((f"{name}_{H}x{W}", plane, thr, want))
    return out


@functools.lru_cache(maxsize=None)
def batch_case():
    """Three different contents in one batch (45 x 70) with the restatement's field of each."""
    from comfyui_sdmatte_amd.sdmatte_nodes import distance_field
    c = {n: p for n, p, _ in contents(45, 70)}
    plane = np.stack([c["blobs"], c["checkerboard"], c["corner_pixel"]])
    return plane, distance_field(torch.from_numpy(plane), 0.5).numpy()


def run_counted(eng, kind, call):
    """The call's result, with the documented launches of its kind counted once each and nothing else launched."""
    eng.lib.kernel_counts(reset=True)
    got = call()
    counts = eng.lib.kernel_counts()
    assert counts == {k: 1 for k in DF_KERNELS[kind]}, counts
    return got


def check_field(eng, to_tensor, cases):
    for name, plane, thr, want in cases:
        t = to_tensor(torch.from_numpy(plane))
        got = run_counted(eng, "field", lambda: eng.distance_field(t, thr))
        assert got.dtype == torch.int32 and tuple(got.shape) == plane.shape and got.device == t.device, name
        got = got.cpu().numpy()
        assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} of {want.size} pixels differ"
        assert int(np.abs(got.astype(np.int64)).min()) >= 1, name


def check_field_batch(eng, to_tensor):
    plane, want = batch_case()
    got = eng.distance_field(to_tensor(torch.from_numpy(plane)), 0.5).cpu().numpy()
    assert np.array_equal(got, want)
    for b in range(3):
        one = eng.distance_field(to_tensor(torch.from_numpy(plane[b:b + 1].copy())), 0.5).cpu().numpy()
        assert np.array_equal(one, got[b:b + 1]), b
    assert len({got[b].tobytes() for b in range(3)}) == 3


def trimap_from_field(field, erode_px, dilate_px):
    out = np.full(field.shape, 0.5, np.float32)
    out[field.astype(np.int64) > erode_px * erode_px] = 1.0
    out[field.astype(np.int64) < -dilate_px * dilate_px] = 0.0
    return out


def check_field_against_trimap(eng, to_tensor, H, W, radii):
    """make_trimap (the capped kernels of csrc/k_trimap.h) equals, bit for bit, the trimap built from the field."""
    mask = TS.blobs(H + W, 1, H, W)
    t = to_tensor(torch.from_numpy(mask))
    field = eng.distance_field(t, 0.5).cpu().numpy()
    for e, d in radii:
        tri = eng.make_trimap(t, 0.5, e, d).cpu().numpy()
        assert np.array_equal(tri, trimap_from_field(field, e, d)), (H, W, e, d)


# ---- sdm_offset_mask / sdm_outline against the fp64 restatement ---------------------------------------------------------------------------
def _compare(name, got, r64, r32):
    """One output tensor under the rule; prints d32 and the deviation."""
    d32 = float((r32.double() - r64).abs().max())
    tol = GS.tolerance(d32)
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == r64.shape and bool(torch.isfinite(got).all()), name
    d = float((got.double() - r64).abs().max())
    print(f"[edge] {name}: d32 = {d32:.3e} tol = {tol:.3e} d = {d:.3e}")
    assert d <= tol, f"{name}: |out - fp64| = {d:.3e} above {tol:.3e} (d32 = {d32:.3e})"


@functools.lru_cache(maxsize=None)
def offset_cases():
    """[(name, mask [B,H,W], threshold, offset_px, feather_px, fp64 reference, fp32 reference)]"""
    from comfyui_sdmatte_amd.sdmatte_nodes import offset_mask
    out = []
    for (H, W), B in (((96, 128), 2), ((130, 257), 1)):
        mask = torch.from_numpy(TS.blobs(H + 3 * W, B, H, W))
        for thr, off, fe in ((0.5, 0.0, 1.0), (0.5, 7.0, 1.0), (0.5, -3.0, 1.0), (0.5, 40.0, 12.5), (0.3, 2.5, 3.0), (0.6, -10.25, 4.0), (0.5, 1024.0, 1024.0),
                             (0.5, -1024.0, 1.0)):
            out.append((f"offset_{H}x{W}_thr{thr}_o{off}_f{fe}", mask, thr, off, fe, offset_mask(mask, off, fe, thr, dtype=torch.float64),
                        offset_mask(mask, off, fe, thr)))
    for name, mask in (("empty", torch.zeros(1, 45, 70)), ("full", torch.ones(1, 45, 70))):
        out.append((f"offset_{name}", mask, 0.5, 5.0, 2.0, offset_mask(mask, 5.0, 2.0, 0.5, dtype=torch.float64), offset_mask(mask, 5.0, 2.0, 0.5)))
    return out


def check_offset_mask(eng, to_tensor):
    for name, mask, thr, off, fe, r64, r32 in offset_cases():
        t = to_tensor(mask)
        got = run_counted(eng, "offset", lambda: eng.offset_mask(t, off, fe, thr))
        assert got.device == t.device, name
        _compare(name, got, r64, r32)
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0, name


@functools.lru_cache(maxsize=None)
def wide_case():
    """12 x 2500: a clump and two seeds, with room for a radius of 1024 on either side of the clump; (mask, its field as int64)."""
    from comfyui_sdmatte_amd.sdmatte_nodes import distance_field
    mask = np.zeros((1, 12, 2500), np.float32)
    mask[0, 4:7, 1200:1204] = 1.0
    mask[0, 0, 60] = mask[0, 11, 2440] = 0.8
    field = distance_field(torch.from_numpy(mask), 0.5).numpy().astype(np.int64)
    return mask, field


def check_offset_mask_exact_consequences(eng, to_tensor, radii=(0, 1, 7, 255, 1024)):
    """(0, 1) is the binarised mask; an integer offset r with feather 1 is exactly 1.0 on d2 <= r^2 (and on F) and above 0 exactly where d2 < (r + 1)^2."""
    from comfyui_sdmatte_amd.sdmatte_nodes import distance_field
    blobs = TS.blobs(5, 1, 130, 257)
    for mask, field in (wide_case(), (blobs, distance_field(torch.from_numpy(blobs), 0.5).numpy().astype(np.int64))):
        t = to_tensor(torch.from_numpy(mask))
        fg = field > 0
        d2 = np.where(fg, 0, -field)
        for r in radii:
            got = eng.offset_mask(t, float(r), 1.0, 0.5).cpu().numpy()
            assert np.array_equal(got == 1.0, d2 <= r * r), (mask.shape, r)
            assert np.array_equal(got > 0.0, d2 < (r + 1) * (r + 1)), (mask.shape, r)
            if r == 0:
                assert np.array_equal(got, fg.astype(np.float32)), mask.shape


def outline_inputs(H=96, W=128, B=2, seed=3):
    """A soft alpha (blobs, exact zeros far outside, a NaN and an out-of-range value) and random foreground colours."""
    alpha = TS.blobs(seed, B, H, W, n=3)
    alpha[alpha < 0.05] = 0.0
    alpha[0, 0, 0] = np.nan
    alpha[0, H // 2, W // 2] = 1.5
    fg = torch.rand(B, H, W, 3, generator=torch.Generator().manual_seed(seed))
    return fg, torch.from_numpy(alpha)


@functools.lru_cache(maxsize=None)
def outline_cases():
    """[(name, fg, alpha, kwargs, (rgb64, a64), (rgb32, a32))]: all three positions, a fractional width, soft and hard, an empty and a full silhouette."""
    from comfyui_sdmatte_amd.sdmatte_nodes import outline_cutout
    fg, alpha = outline_inputs()
    fg2, alpha2 = outline_inputs(130, 257, 1, seed=8)
    out = []
    for name, f, a, kw in (
            ("outside_hard", fg, alpha, dict(width_px=5.0, color=(1.0, 0.5, 0.0), position="outside")),
            ("outside_soft_fractional", fg, alpha, dict(width_px=6.5, color=(0.1, 0.9, 0.3), position="outside", softness_px=3.25, opacity=0.7, edge_threshold=0.3)),
            ("center", fg, alpha, dict(width_px=7.0, color=(0.0, 0.0, 1.0), position="center", softness_px=1.5, opacity=0.85)),
            ("inside_fractional", fg, alpha, dict(width_px=4.75, color=(1.0, 1.0, 1.0), position="inside", softness_px=2.0)),
            ("inside_2", fg, alpha, dict(width_px=9.0, color=(0.2, 0.2, 0.2), position=2, opacity=0.5)),
            ("wide_130x257", fg2, alpha2, dict(width_px=40.0, color=(1.0, 0.0, 1.0), position="outside", softness_px=12.0)),
            ("center_130x257", fg2, alpha2, dict(width_px=3.0, color=(0.3, 0.6, 0.9), position=1)),
            ("empty_silhouette", fg, torch.zeros_like(alpha), dict(width_px=5.0, color=(1.0, 0.0, 0.0), position="outside")),
            ("empty_silhouette_inside", fg, torch.zeros_like(alpha), dict(width_px=5.0, color=(1.0, 0.0, 0.0), position="inside")),
            ("full_silhouette", fg, torch.full_like(alpha, 0.75), dict(width_px=5.0, color=(1.0, 0.0, 0.0), position="center")),
            ("full_silhouette_outside", fg, torch.ones_like(alpha), dict(width_px=1024.0, color=(1.0, 0.0, 0.0), position="outside", softness_px=1024.0))):
        out.append((name, f, a, kw, outline_cutout(f, a, dtype=torch.float64, **kw), outline_cutout(f, a, **kw)))
    return out


def check_outline(eng, to_tensor):
    for name, fg, alpha, kw, r64, r32 in outline_cases():
        f, a = to_tensor(fg), to_tensor(alpha)
        rgb, A = run_counted(eng, "outline", lambda: eng.outline(f, a, **kw))
        assert rgb.device == f.device and A.device == f.device, name
        _compare(name + " alpha", A, r64[1], r32[1])
        _compare(name + " rgb", rgb, r64[0], r32[0])


def check_outline_exact_properties(eng, to_tensor):
    """Position 0, opacity 1, softness 1: alpha == 1.0 on the closed-disk dilation of the silhouette, and the subject's own alpha from width + 1 outwards;
    opacity 0 returns the subject layer, in every position."""
    from comfyui_sdmatte_amd.sdmatte_nodes import distance_field
    fg, alpha = outline_inputs()
    f, a = to_tensor(fg), to_tensor(alpha)
    a_clean = torch.nan_to_num(alpha, nan=0.0).clamp(0.0, 1.0)
    for thr, width in ((0.5, 5), (0.3, 12)):
        field = distance_field(alpha, thr).numpy().astype(np.int64)
        d2 = np.where(field > 0, 0, -field)
        rgb, A = eng.outline(f, a, float(width), (0.0, 1.0, 0.0), "outside", 1.0, 1.0, thr)
        A = A.cpu().numpy()
        assert bool((A[d2 <= width * width] == 1.0).all()), (thr, width)
        sd = np.sqrt(d2.astype(np.float64)) - 0.5
        far = (field < 0) & (sd >= width + 1)
        assert far.any() and np.array_equal(A[far], a_clean.numpy()[far]), (thr, width)
    for position in ("outside", "center", "inside"):
        rgb, A = eng.outline(f, a, 6.0, (1.0, 0.0, 0.0), position, 2.0, 0.0, 0.5)
        assert torch.equal(A.cpu(), a_clean), position
        keep = a_clean > 0
        assert torch.equal(rgb.cpu()[keep], fg[keep]), position
        assert bool((rgb.cpu()[~keep] == 0).all()), position


# ---- the calls' contract ------------------------------------------------------------------------------------------------------------------
def check_errors(eng, to_tensor):
    """Python raises ValueError; the raw C calls return SDM_ERR_INVALID (-1) with a message and leave the outputs alone."""
    import pytest
    from comfyui_sdmatte_amd.engine import _ptr
    import ctypes as C
    p = to_tensor(torch.rand(1, 20, 30))
    fg = to_tensor(torch.rand(1, 20, 30, 3))
    nan, inf = float("nan"), float("inf")
    for bad in (dict(threshold=1.0), dict(threshold=-0.5), dict(threshold=nan), dict(threshold=inf), dict(threshold=1.0 - 1e-9)):
        with pytest.raises(ValueError):
            eng.distance_field(p, **bad)
        with pytest.raises(ValueError):
            eng.offset_mask(p, 1.0, 1.0, **bad)
        with pytest.raises(ValueError):
            eng.outline(fg, p, edge_threshold=bad["threshold"])
    for bad in (dict(offset_px=1024.5), dict(offset_px=-1025.0), dict(offset_px=nan), dict(offset_px=inf), dict(feather_px=0.5), dict(feather_px=0.0),
                dict(feather_px=1024.5), dict(feather_px=nan), dict(feather_px=-1.0)):
        with pytest.raises(ValueError):
            eng.offset_mask(p, **bad)
    for bad in (dict(width_px=0.0), dict(width_px=-1.0), dict(width_px=1024.5), dict(width_px=nan), dict(softness_px=0.5), dict(softness_px=1025.0),
                dict(softness_px=inf), dict(opacity=-0.1), dict(opacity=1.1), dict(opacity=nan), dict(position=3), dict(position=-1), dict(position="around"),
                dict(position=1.5), dict(color=(1.0, 1.0)), dict(color=(1.0, nan, 0.0))):
        with pytest.raises(ValueError):
            eng.outline(fg, p, **bad)
    for call in (lambda: eng.distance_field(p[0]), lambda: eng.distance_field(p[:, :0]), lambda: eng.offset_mask(p[0]), lambda: eng.outline(fg[..., :2], p),
                 lambda: eng.outline(fg, p[:, :10]), lambda: eng.distance_field(p, out=torch.empty(1, 20, 30, device=p.device)),
                 lambda: eng.offset_mask(p, out=torch.empty(1, 20, 30, dtype=torch.int32, device=p.device)),
                 lambda: eng.outline(fg, p, out=(torch.empty(1, 20, 30, device=p.device), torch.empty(1, 20, 30, device=p.device)))):
        with pytest.raises(ValueError):
            call()
    kind = eng._kind(p)
    field = torch.full((1, 20, 30), -7, dtype=torch.int32, device=p.device)
    out = torch.full((1, 20, 30), -7.0, device=p.device)
    out_rgb = torch.full((1, 20, 30, 3), -7.0, device=p.device)
    rgb = (C.c_float * 3)(1.0, 1.0, 1.0)
    bad_rgb = (C.c_float * 3)(1.0, nan, 1.0)
    lib, h = eng.lib, eng.h

    def field_rc(B=1, H=20, W=30, thr=0.5, k=kind):
        return lib.sdm_distance_field(h, _ptr(p), B, H, W, thr, _ptr(field), k, None)

    def offset_rc(B=1, H=20, W=30, thr=0.5, off=1.0, fe=1.0, k=kind):
        return lib.sdm_offset_mask(h, _ptr(p), B, H, W, thr, off, fe, _ptr(out), k, None)

    def outline_rc(B=1, H=20, W=30, thr=0.5, pos=0, width=2.0, soft=1.0, col=rgb, op=1.0, k=kind):
        return lib.sdm_outline(h, _ptr(fg), _ptr(p), B, H, W, thr, pos, width, soft, col, op, _ptr(out_rgb), _ptr(out), k, None)

    for rc_of in (field_rc, offset_rc, outline_rc):
        for kw, msg in ((dict(thr=1.0), b"threshold"), (dict(thr=nan), b"threshold"), (dict(thr=-0.25), b"threshold"), (dict(thr=inf), b"threshold"),
                        (dict(B=0), b"bad plane size"), (dict(H=0), b"bad plane size"), (dict(W=0), b"bad plane size"), (dict(W=40000), b"too large"),
                        (dict(B=16, H=32768, W=32768), b"too large"), (dict(k=7), b"ptr_kind")):
            assert rc_of(**kw) == -1 and msg in lib.sdm_last_error(h), (rc_of.__name__, kw, lib.sdm_last_error(h))
    for kw, msg in ((dict(off=1024.5), b"offset_px"), (dict(off=-1024.5), b"offset_px"), (dict(off=nan), b"offset_px"), (dict(off=inf), b"offset_px"),
                    (dict(fe=0.5), b"feather_px"), (dict(fe=1024.5), b"feather_px"), (dict(fe=nan), b"feather_px")):
        assert offset_rc(**kw) == -1 and msg in lib.sdm_last_error(h), (kw, lib.sdm_last_error(h))
    for kw, msg in ((dict(pos=3), b"position"), (dict(pos=-1), b"position"), (dict(width=0.0), b"width_px"), (dict(width=1024.5), b"width_px"),
                    (dict(width=nan), b"width_px"), (dict(soft=0.5), b"softness_px"), (dict(soft=1024.5), b"softness_px"), (dict(soft=inf), b"softness_px"),
                    (dict(op=-0.1), b"opacity"), (dict(op=1.5), b"opacity"), (dict(op=nan), b"opacity"), (dict(col=bad_rgb), b"rgb3")):
        assert outline_rc(**kw) == -1 and msg in lib.sdm_last_error(h), (kw, lib.sdm_last_error(h))
    assert lib.sdm_outline(h, _ptr(fg), _ptr(p), 1, 20, 30, 0.5, 0, 2.0, 1.0, None, 1.0, _ptr(out_rgb), _ptr(out), kind, None) == -1      # no colour
    eng.synchronize()
    assert bool((field == -7).all()) and bool((out == -7).all()) and bool((out_rgb == -7).all())
    assert eng.distance_field(p, out=field) is field and bool((field != -7).all())
    assert eng.offset_mask(p, out=out) is out and bool((out != -7).all())
    got = eng.outline(fg, p, out=(out_rgb, out))
    assert got[0] is out_rgb and got[1] is out and bool((out_rgb != -7).all())


def check_memory(eng, to_tensor, H=64, W=96):
    """What the calls keep is counted by resident_bytes and given back by release_memory; an engine without weights runs them."""
    eng.release_memory()
    assert eng.resident_bytes() == eng.weight_bytes()
    p = to_tensor(torch.rand(2, H, W))
    eng.distance_field(p)
    mid = eng.resident_bytes()
    nt = (H + 31) // 32
    assert mid >= eng.weight_bytes() + 2 * H * W * 2 + 2 * nt * W * 20      # the column distances, the class words and the carries (arena)
    from comfyui_sdmatte_amd.engine import SDM_PTR_HOST
    if eng._kind(p) == SDM_PTR_HOST:
        assert mid >= eng.weight_bytes() + 2 * H * W * (2 + 4 + 4)          # ... and the staging in and out
    eng.outline(to_tensor(torch.rand(2, H, W, 3)), p)
    assert eng.resident_bytes() >= mid
    eng.release_memory()
    assert eng.resident_bytes() == eng.weight_bytes()
    eng.offset_mask(p, 3.0, 2.0)                                            # ... and the next call allocates again
    assert eng.resident_bytes() > eng.weight_bytes()
