"""Shared by tests/test_emu_tiles.py and tests/test_gpu_tiles.py: the cases of the tiles along the unknown band (sdm_band_tiles) with a brute force written
from the definition in include/sdmatte.h - the grid by the rule in Python integers, any() over every tile's rectangle; it shares no code with the kernels
(csrc/k_tiles.h) or with the CPU restatement (sdmatte_nodes.band_tiles, which counts through a summed-area table) - and the compositions of existing calls
that sdm_apply_matte_tiles must equal: exactly where a pixel lies in one tile, within TOL where several are blended."""
import ctypes

import numpy as np
import torch

import boxes_suite as BS
import roi_suite as RS

VOID = [-1, 0, 0, 0, 0]
BAND_KERNELS = ("tiles_init", "tiles_mark", "tiles_list")
CALL_KERNELS = ("boxes_sanitize", "boxes_prep_image", "boxes_prep_trimap", "tiles_blend")
MAX_GRID = 256
H_E2E, W_E2E, S_E2E, C_E2E = RS.H_E2E, RS.W_E2E, RS.S_E2E, RS.C_E2E
# Both sides evaluate sum (w_i / Wsum) * a_i on bit-identical a_i and w_i and may differ only in fused against unfused multiply-add: each side's relative
# error is at most (2n + 1) * 2^-24 for n <= 16 covering tiles and the values lie in [0, 1], so they differ by less than 66 * 2^-24 < 2^-18.
TOL = 2.0 ** -18


# ---- reference --------------------------------------------------------------------------------------------------------------------------
def axis(L, T, O):
    """(origins, size) of one axis by the rule."""
    if L <= T:
        return [0], L
    n = -(-(L - O) // (T - O))
    return [(i * (L - T)) // (n - 1) for i in range(n)], T


def grid_cells(H, W, T, O):
    return len(axis(H, T, O)[0]) * len(axis(W, T, O)[0])


def brute_force(plane, lo, hi, T, O, K):
    """(tiles int32 [B,K,5], count int32 [B]) from the definition."""
    B, H, W = plane.shape
    (oy, sy), (ox, sx) = axis(H, T, O), axis(W, T, O)
    out = np.zeros((B, K, 5), np.int32)
    out[:, :, 0] = -1
    count = np.zeros(B, np.int32)
    for b in range(B):
        with np.errstate(invalid="ignore"):
            band = (np.float32(lo) < plane[b]) & (plane[b] < np.float32(hi))
        n = 0
        for y0 in oy:
            for x0 in ox:
                if band[y0:y0 + sy, x0:x0 + sx].any():
                    if n < K:
                        out[b, n] = (b, y0, x0, sy, sx)
                    n += 1
        count[b] = n
    return out, count


def band_covered(plane, lo, hi, tiles):
    """Every band pixel lies in at least one listed tile of its image."""
    B, H, W = plane.shape
    for b in range(B):
        cover = np.zeros((H, W), bool)
        for bb, y0, x0, h, w in tiles[b].tolist():
            if bb >= 0:
                assert bb == b and 0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= H and x0 + w <= W, (b, bb, y0, x0, h, w)
                cover[y0:y0 + h, x0:x0 + w] = True
        with np.errstate(invalid="ignore"):
            if bool(((np.float32(lo) < plane[b]) & (plane[b] < np.float32(hi)) & ~cover).any()):
                return False
    return True


# ---- planes -----------------------------------------------------------------------------------------------------------------------------
def ring(H, W, B=1, cy=0.5, cx=0.5, r=0.35, width=0.08):
    """1.0 inside an ellipse, 0.0 outside, 0.5 in a band around its outline (a subject with an unknown rim)."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.sqrt(((y + 0.5) / H - cy) ** 2 + ((x + 0.5) / W - cx) ** 2)
    p = np.where(d < r - width / 2, 1.0, np.where(d < r + width / 2, 0.5, 0.0)).astype(np.float32)
    return np.repeat(p[None], B, 0)


def dots(H, W, points, value=0.5, bg=0.0):
    p = np.full((1, H, W), bg, np.float32)
    for y, x in points:
        p[0, y, x] = value
    return p


SHAPES = [(1, 1), (1, 300), (257, 3), (96, 128), (97, 131), (150, 200), (300, 517)]      # 300 x 517: several blocks, W % 4 != 0; 96 x 128: the vector path
PAIRS = [(64, 16), (64, 0), (64, 32), (80, 16), (16, 8)]


def band_cases(big=False):
    """[(name, plane fp32 [B,H,W], band_lo, band_hi, tile, overlap, max_tiles)] - the issue's list.  A (tile, overlap) pair is run on every shape whose
    grid it keeps within SDM_TILES_MAX_GRID cells."""
    out = []
    for H, W in SHAPES:
        for T, O in PAIRS:
            if grid_cells(H, W, T, O) > MAX_GRID:
                continue
            out.append((f"ring_{H}x{W}_T{T}_O{O}", ring(H, W), 0.25, 0.75, T, O, 16))
    H, W, T, O = 150, 200, 64, 16
    (oy, _), (ox, _) = axis(H, T, O), axis(W, T, O)
    assert (oy, ox) == ([0, 43, 86], [0, 45, 90, 136])
    out.append(("empty_band", np.where(ring(H, W) > 0.75, 1.0, 0.0).astype(np.float32), 0.25, 0.75, T, O, 16))
    out.append(("every_pixel_in_the_band", np.full((1, H, W), 0.5, np.float32), 0.25, 0.75, T, O, 16))
    for name, pt in (("top_left", (0, 0)), ("top_right", (0, W - 1)), ("bottom_left", (H - 1, 0)), ("bottom_right", (H - 1, W - 1))):
        out.append((f"single_pixel_{name}", dots(H, W, [pt]), 0.25, 0.75, T, O, 16))
    for iy, y0 in enumerate(oy):
        for ix, x0 in enumerate(ox):
            # the first and the last pixel of tile (iy, ix), and their neighbours just outside it: off-by-one in the ranges shows as one tile more or less
            for tag, pt in (("first", (y0, x0)), ("last", (y0 + T - 1, x0 + T - 1)), ("before", (max(y0 - 1, 0), max(x0 - 1, 0))),
                            ("behind", (min(y0 + T, H - 1), min(x0 + T, W - 1)))):
                out.append((f"single_pixel_{tag}_of_tile_{iy}_{ix}", dots(H, W, [pt], bg=1.0), 0.25, 0.75, T, O, 16))
    edge = ring(H, W)
    edge[edge == 0.5] = 0.25                                                       # exactly band_lo: outside
    edge[0, 100:110, 20:30] = 0.75                                                 # exactly band_hi: outside
    edge[0, 5:9, 190:195] = np.nan
    out.append(("bounds_and_nan_are_outside", edge, 0.25, 0.75, T, O, 16))
    edge2 = edge.copy()
    edge2[0, 120, 150] = np.nextafter(np.float32(0.25), np.float32(1.0))            # the next fp32 above band_lo: inside
    out.append(("next_float_above_lo_is_inside", edge2, 0.25, 0.75, T, O, 16))
    out.append(("other_band", ring(H, W) * np.float32(0.9), 0.4, 0.5, T, O, 16))
    two = np.concatenate([ring(H, W, cy=0.3, cx=0.3, r=0.2), dots(H, W, [(149, 0), (70, 100)]), np.zeros((1, H, W), np.float32)])
    out.append(("batch_of_three_different_content", two, 0.25, 0.75, T, O, 16))
    for K in (1, 3, 7):
        out.append((f"max_tiles_{K}_below_the_count", ring(H, W), 0.25, 0.75, T, O, K))
    out.append(("overflow_of_sixteen", np.full((1, 97, 131), 0.5, np.float32), 0.25, 0.75, 16, 8, 16))
    out.append(("three_tiles_per_axis_113", dots(113, 113, [(50, 50)]), 0.25, 0.75, 64, 16, 16))
    out.append(("three_tiles_per_axis_113_ring", ring(113, 113), 0.25, 0.75, 64, 16, 16))
    if big:
        pl = np.concatenate([ring(1080, 1920), ring(1080, 1920, cy=0.2, cx=0.8, r=0.15, width=0.01)])
        pl[1, 1079, 0] = 0.5
        out.append(("many_blocks_1080x1920", pl, 0.25, 0.75, 512, 64, 16))
    return out


def check_band_tiles(eng, to_tensor, cases=None):
    """eng.band_tiles equals the brute force and the CPU restatement in every case, with the same three launches each; the list covers every band pixel
    unless it overflows; void entries behind the active ones; every image of a batch equals its own single-image call."""
    from comfyui_sdmatte_amd.sdmatte_nodes import band_tiles
    for name, plane, lo, hi, T, O, K in (cases if cases is not None else band_cases()):
        t = to_tensor(torch.from_numpy(plane))
        B = plane.shape[0]
        eng.lib.kernel_counts(reset=True)
        got, cnt = eng.band_tiles(t, lo, hi, T, O, K, return_count=True)
        counts = eng.lib.kernel_counts()
        assert counts == {k: 1 for k in BAND_KERNELS}, (name, counts)
        assert got.dtype == torch.int32 and tuple(got.shape) == (B, K, 5) and got.device == t.device and cnt.dtype == torch.int32 and tuple(cnt.shape) == (B, ), name
        want, wcnt = brute_force(plane, lo, hi, T, O, K)
        g, c = got.cpu().numpy(), cnt.cpu().numpy()
        assert np.array_equal(g, want) and np.array_equal(c, wcnt), (name, g.tolist(), want.tolist(), c.tolist(), wcnt.tolist())
        rb, rc = band_tiles(torch.from_numpy(plane), lo, hi, T, O, K, return_count=True)
        assert np.array_equal(g, rb.numpy()) and np.array_equal(c, rc.numpy()), name
        for b in range(B):
            n = min(int(c[b]), K)
            assert all(e == VOID for e in g[b, n:].tolist()) and all(e[0] == b for e in g[b, :n].tolist()), (name, g.tolist())
        if int(c.max()) <= K:
            assert band_covered(plane, lo, hi, g), name
        if B > 1:
            for b in range(B):
                single = eng.band_tiles(to_tensor(torch.from_numpy(plane[b:b + 1])), lo, hi, T, O, K).cpu()
                assert torch.equal(got[b, :, 1:].cpu(), single[0, :, 1:]), (name, b)


def check_cases_mean_what_their_names_say():
    cases = {c[0]: c for c in band_cases()}
    assert len(cases) == len(band_cases())

    def run(name):
        _, plane, lo, hi, T, O, K = cases[name]
        return brute_force(plane, lo, hi, T, O, K)
    assert run("empty_band")[1].tolist() == [0] and run("every_pixel_in_the_band")[1].tolist() == [12] and run("bounds_and_nan_are_outside")[1].tolist() == [0]
    assert run("next_float_above_lo_is_inside")[1].tolist() == [2]                 # (120, 150): y tile 2, x tiles 2 and 3
    assert run("single_pixel_top_left")[0][0, 0].tolist() == [0, 0, 0, 64, 64] and run("single_pixel_bottom_right")[0][0, 0].tolist() == [0, 86, 136, 64, 64]
    assert run("three_tiles_per_axis_113")[1].tolist() == [9]
    assert run("max_tiles_3_below_the_count")[1].tolist() == run("max_tiles_7_below_the_count")[1].tolist() and run("max_tiles_3_below_the_count")[1][0] > 7
    assert run("overflow_of_sixteen")[1].tolist() == [192]
    c = run("batch_of_three_different_content")[1].tolist()
    assert c[2] == 0 and c[0] > 0 and c[1] == 1 + 2                                # (149, 0): one tile; (70, 100): y tile 1, x tiles 1 and 2


def check_band_tiles_errors(eng, to_tensor):
    """Python raises ValueError; the raw C call returns SDM_ERR_INVALID (-1) with a message that names the argument and leaves the outputs alone."""
    import pytest
    from comfyui_sdmatte_amd.engine import _ptr
    p = to_tensor(torch.rand(1, 40, 50))
    for bad in (dict(band_lo=-0.1), dict(band_lo=0.75), dict(band_lo=0.8), dict(band_hi=1.5), dict(band_lo=float("nan")), dict(band_hi=float("inf")),
                dict(tile=15), dict(tile=32769), dict(tile=64.5), dict(overlap=-1), dict(overlap=513), dict(tile=64, overlap=33), dict(max_tiles=0),
                dict(max_tiles=17), dict(max_tiles=2.5), dict(max_tiles=-1)):
        with pytest.raises(ValueError):
            eng.band_tiles(p, **bad)
    with pytest.raises(ValueError):
        eng.band_tiles(p[0])
    with pytest.raises(ValueError):
        eng.band_tiles(to_tensor(torch.rand(1, 150, 200)), tile=16, overlap=8)                  # 18 x 24 cells
    with pytest.raises(ValueError):
        eng.band_tiles(p, out=torch.empty(1, 4, 5, dtype=torch.int32, device=p.device))
    out = torch.full((1, 4, 5), -7, dtype=torch.int32, device=p.device)
    cnt = torch.full((1, ), -7, dtype=torch.int32, device=p.device)
    kind = eng._kind(p)
    for args, msg in (((0.75, 0.75, 64, 16, 4), b"band_lo"), ((-0.5, 0.75, 64, 16, 4), b"band_lo"), ((0.25, 1.5, 64, 16, 4), b"band_hi"),
                      ((float("nan"), 0.75, 64, 16, 4), b"band_lo"), ((0.25, 0.75, 15, 4, 4), b"tile = 15"), ((0.25, 0.75, 32769, 4, 4), b"tile = 32769"),
                      ((0.25, 0.75, 64, -1, 4), b"overlap"), ((0.25, 0.75, 64, 33, 4), b"overlap"), ((0.25, 0.75, 64, 16, 0), b"max_tiles"),
                      ((0.25, 0.75, 64, 16, 17), b"max_tiles")):
        rc = eng.lib.sdm_band_tiles(eng.h, _ptr(p), 1, 40, 50, *args, _ptr(out), _ptr(cnt), kind, None)
        assert rc == -1 and msg in eng.lib.sdm_last_error(eng.h), (args, rc, eng.lib.sdm_last_error(eng.h))
    big = to_tensor(torch.rand(1, 150, 200))
    assert eng.lib.sdm_band_tiles(eng.h, _ptr(big), 1, 150, 200, 0.25, 0.75, 16, 8, 4, _ptr(out), _ptr(cnt), kind, None) == -1
    assert b"grid" in eng.lib.sdm_last_error(eng.h)
    assert eng.lib.sdm_band_tiles(eng.h, _ptr(p), 1, 0, 50, 0.25, 0.75, 64, 16, 4, _ptr(out), _ptr(cnt), kind, None) == -1
    assert eng.lib.sdm_band_tiles(eng.h, _ptr(p), 1, 40, 40000, 0.25, 0.75, 64, 16, 4, _ptr(out), _ptr(cnt), kind, None) == -1
    assert eng.lib.sdm_band_tiles(eng.h, _ptr(p), 1, 40, 50, 0.25, 0.75, 64, 16, 4, _ptr(out), _ptr(cnt), 7, None) == -1
    eng.synchronize()
    assert bool((out == -7).all()) and bool((cnt == -7).all())
    got = eng.band_tiles(p, max_tiles=4, out=out)
    assert got is out and not bool((out == -7).any())


# ---- sdm_apply_matte_tiles ----------------------------------------------------------------------------------------------------------------
def tiles_tensor(entries):
    return torch.tensor(entries, dtype=torch.int32).reshape(-1, 5)


def call(eng, to_tensor, image, trimap, tiles, mode="alpha_only", refine=False, feather=None, base=None, **kw):
    return eng.apply_matte_tiles(to_tensor(image), to_tensor(trimap), to_tensor(tiles), S_E2E, False, mode, refine, C_E2E, feather,
                                 None if base is None else to_tensor(base), **kw)


def count_once(eng, fn, kernels=CALL_KERNELS):
    """Runs fn() and asserts that each of the call's own kernels was launched exactly once, and no boxes_paste (sdm_kernel_counts)."""
    eng.lib.kernel_counts(reset=True)
    out = fn()
    counts = eng.lib.kernel_counts()
    assert {k: v for k, v in counts.items() if k.startswith(("boxes_", "tiles_", "roi_"))} == {k: 1 for k in kernels}, counts
    return out


def definite(trimap):
    """The base of a call without one: 1.0 where trimap > 0.5, else 0.0."""
    return (trimap > 0.5).float()


def crops_of(eng, to_tensor, image, trimap, tiles):
    """Crops by hand and ONE apply_matte_node call of batch N on them (alpha_only, no refine; so all tiles have one size)."""
    ic = torch.stack([image[b, y0:y0 + h, x0:x0 + w] for b, y0, x0, h, w in tiles.tolist()]).contiguous()
    tc = torch.stack([trimap[b, y0:y0 + h, x0:x0 + w] for b, y0, x0, h, w in tiles.tolist()]).contiguous()
    crops, _ = eng.apply_matte_node(to_tensor(ic), to_tensor(tc), S_E2E, False, "alpha_only", False, C_E2E)
    return crops.cpu()


def coverage(tiles, B, H, W):
    n = torch.zeros(B, H, W, dtype=torch.int32)
    for b, y0, x0, h, w in tiles.tolist():
        n[b, y0:y0 + h, x0:x0 + w] += 1
    return n


def check_equals_composition(eng, to_tensor, image, trimap, tiles, feather, modes, base=None, exact=False, crops=None):
    """The call against crops + sdmatte_nodes.blend_tiles + refine_and_compose: torch.equal with `exact` (single coverage), else within TOL - and then
    the crops that meet in a pixel must really differ somewhere, so that the weights are exercised.  Returns the crops."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    B, H, W = trimap.shape
    if crops is None:
        crops = crops_of(eng, to_tensor, image, trimap, tiles)
    blended = N.blend_tiles(crops, tiles, B, H, W, feather, definite(trimap) if base is None else base)
    cover = coverage(tiles, B, H, W)
    assert (int(cover.max()) == 1) == exact, int(cover.max())
    for mode, refine in modes:
        alpha, matted = N.refine_and_compose(blended, image, trimap, mode, refine, C_E2E)
        a, m = count_once(eng, lambda: call(eng, to_tensor, image, trimap, tiles, mode, refine, feather, base))
        a, m = a.cpu(), m.cpu()
        if exact:
            assert torch.equal(a, alpha) and torch.equal(m, matted), (mode, refine, float((a - alpha).abs().max()))
        else:
            da, dm = float((a - alpha).abs().max()), float((m - matted).abs().max())
            print(f"tiles composition {tuple(trimap.shape)} N={tiles.shape[0]} feather={feather} {mode} refine={refine}: max |alpha diff| {da:.3g}, "
                  f"max |matted diff| {dm:.3g} (bound {TOL:.3g})")
            assert da <= TOL and dm <= TOL, (mode, refine, da, dm)
            single = cover == 1
            if not refine:
                assert torch.equal(a[single], blended[single])                          # single coverage is exact inside an overlapping list too
    if not exact:
        differ = False
        ent = tiles.tolist()
        for i in range(len(ent)):
            for j in range(i + 1, len(ent)):
                (bi, yi, xi, hi, wi), (bj, yj, xj, hj, wj) = ent[i], ent[j]
                y0, y1, x0, x1 = max(yi, yj), min(yi + hi, yj + hj), max(xi, xj), min(xi + wi, xj + wj)
                if bi == bj and y0 < y1 and x0 < x1:
                    ca, cb = crops[i][y0 - yi:y1 - yi, x0 - xi:x1 - xi], crops[j][y0 - yj:y1 - yj, x0 - xj:x1 - xj]
                    differ = differ or (bool((ca > cb).any()) and bool((cb > ca).any()))
        assert differ
    return crops


def soft_trimap(B, H, W, regions, seed):
    """Definite 0.0 / 1.0 by the blobs of boxes_suite.frames, except inside the rectangle (y0, y1, x0, x1) of each image: there the blobs scaled into
    (0.3, 0.7), the unknown band."""
    image, soft = BS.frames(B, seed, H, W)
    tri = (soft > 0.5).float()
    for b, (y0, y1, x0, x1) in enumerate(regions):
        tri[b, y0:y1, x0:x1] = 0.3 + 0.4 * soft[b, y0:y1, x0:x1].clamp(0.0, 1.0)
    return image, tri


def check_equals_node_call(eng, to_tensor, modes=None):
    """One tile = the whole frame: bit-identical to apply_matte_node in alpha and matted, whatever the feather (every side lies on the border)."""
    image, trimap = BS.frames(1, seed=33)
    tiles = tiles_tensor([[0, 0, 0, H_E2E, W_E2E]])
    for mode, refine in (modes or tuple((m, r) for m in ("alpha_only", "matted_rgba", "matted_rgb") for r in (False, True))):
        a, m = eng.apply_matte_node(to_tensor(image), to_tensor(trimap), S_E2E, False, mode, refine, C_E2E)
        a2, m2 = count_once(eng, lambda: call(eng, to_tensor, image, trimap, tiles, mode, refine, 9))
        assert torch.equal(a, a2) and torch.equal(m, m2), (mode, refine, float((a - a2).abs().max()))


def check_disjoint_tiles(eng, to_tensor, modes=None):
    """Two disjoint tiles with a feather: single coverage, so exact in alpha and matted; outside them the base, exactly - the definite trimap, or a base
    plane with NaN and values beyond [0, 1] in it."""
    image, trimap = BS.frames(1, seed=35)
    tiles = tiles_tensor([[0, 5, 8, 40, 48], [0, 50, 70, 40, 48]])
    modes = modes or tuple((m, r) for m in ("alpha_only", "matted_rgba", "matted_rgb") for r in (False, True))
    crops = check_equals_composition(eng, to_tensor, image, trimap, tiles, 5, modes, exact=True)
    base = torch.rand(1, H_E2E, W_E2E, generator=torch.Generator().manual_seed(36)) * 1.5 - 0.25
    base[0, ::9, ::7] = float("nan")
    check_equals_composition(eng, to_tensor, image, trimap, tiles, 5, (("alpha_only", False), ), base=base, exact=True, crops=crops)
    outside = coverage(tiles, 1, H_E2E, W_E2E) == 0
    a, _ = call(eng, to_tensor, image, trimap, tiles, feather=5)
    assert torch.equal(a.cpu()[outside], definite(trimap)[outside])
    a, _ = call(eng, to_tensor, image, trimap, tiles, feather=5, base=base)
    clean = torch.nan_to_num(base, nan=0.0)
    assert torch.equal(a.cpu()[outside], clean.clamp(0, 1)[outside])
    assert float(clean[outside].max()) > 1.0 and float(clean[outside].min()) < 0.0 and bool(torch.isnan(base[outside]).any())


H_OV, W_OV = 150, 200
MODES_OV = (("alpha_only", False), ("matted_rgba", True))


def check_overlapping_tiles(eng, to_tensor, modes64=MODES_OV, modes80=MODES_OV):
    """Lists from band_tiles on a 150 x 200 frame: tile 64, overlap 16, feather 16 (pixels in four tiles); tile 80 (the resample branch)."""
    from comfyui_sdmatte_amd.sdmatte_nodes import band_tiles, compact_boxes
    image, trimap = soft_trimap(1, H_OV, W_OV, ((30, 75, 40, 110), ), seed=37)
    for T, O, feather, n_want, most, modes in ((64, 16, 16, 6, 4, modes64), (80, 16, 11, 6, 6, modes80)):      # (rows 70 .. 74 lie in three tiles of 80)
        tiles = compact_boxes(band_tiles(trimap, 0.25, 0.75, T, O))
        got = compact_boxes(eng.band_tiles(to_tensor(trimap), 0.25, 0.75, T, O))
        assert torch.equal(tiles, got) and tiles.shape[0] == n_want and int(coverage(tiles, 1, H_OV, W_OV).max()) == most, tiles.tolist()
        check_equals_composition(eng, to_tensor, image, trimap, tiles, feather, modes)


def check_mixed_order_and_base(eng, to_tensor, modes=MODES_OV, modes_base=MODES_OV):
    """B = 2, the list of band_tiles in mixed image order, feather 0 (plain averages where tiles meet), with and without a base."""
    from comfyui_sdmatte_amd.sdmatte_nodes import band_tiles, compact_boxes
    image, trimap = soft_trimap(2, H_OV, W_OV, ((30, 75, 40, 70), (100, 140, 120, 180)), seed=39)
    tiles = compact_boxes(band_tiles(trimap, 0.25, 0.75, 64, 16))
    assert sorted(set(tiles[:, 0].tolist())) == [0, 1] and 4 <= tiles.shape[0] <= 8
    tiles = torch.cat([tiles[1::2], tiles[0::2]]).contiguous()
    assert tiles[:, 0].tolist() != sorted(tiles[:, 0].tolist())
    crops = check_equals_composition(eng, to_tensor, image, trimap, tiles, 0, modes)
    base = torch.rand(2, H_OV, W_OV, generator=torch.Generator().manual_seed(40))
    check_equals_composition(eng, to_tensor, image, trimap, tiles, 0, modes_base, base=base, crops=crops)


def check_constant_slots(eng, to_tensor):
    """Equal slot values stay that value under a feather: the weights are normalised before the multiply.  No model promises a constant slot, so the list
    is four times the same S x S tile: every pixel of it blends four equal values a with the weights w_i / Wsum, which gives a up to the rounding of
    the partial sums: |out - a| <= 4 * 2^-24.  (sdmatte_nodes.blend_tiles is checked on constant crops under unequal weights in
    tests/test_node_tiles_cpu.py, and the compositions tie the kernel to it.)"""
    image, trimap = BS.frames(1, seed=41)
    one = [0, 16, 32, S_E2E, S_E2E]
    a1, _ = call(eng, to_tensor, image, trimap, tiles_tensor([one] * 4), feather=13)
    a4 = a1.cpu()[0, 16:16 + S_E2E, 32:32 + S_E2E]
    crops = crops_of(eng, to_tensor, image, trimap, tiles_tensor([one] * 4))
    assert all(torch.equal(crops[0], c) for c in crops[1:])
    d = float((a4 - crops[0]).abs().max())
    print(f"tiles constant slots: max |blend - value| {d:.3g} (bound {4 * 2.0 ** -24:.3g})")
    assert d <= 4 * 2.0 ** -24 and float(crops[0].max()) > float(crops[0].min())


def check_no_tiles(eng, to_tensor):
    """N = 0: no preparation, no model kernel - tiles_blend is the only counted launch - and every pixel is the base, then the tail."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    image, trimap = BS.frames(1, seed=43)
    none = tiles_tensor([])
    assert none.shape == (0, 5)
    eng.lib.kernel_counts(reset=True)
    a, m = call(eng, to_tensor, image, trimap, none, "matted_rgba", True, 8)
    assert eng.lib.kernel_counts() == {"tiles_blend": 1}, eng.lib.kernel_counts()
    alpha, matted = N.refine_and_compose(definite(trimap), image, trimap, "matted_rgba", True, C_E2E)
    assert torch.equal(a.cpu(), alpha) and torch.equal(m.cpu(), matted)
    base = torch.rand(1, H_E2E, W_E2E, generator=torch.Generator().manual_seed(44))
    a, _ = call(eng, to_tensor, image, trimap, none, base=base)
    assert torch.equal(a.cpu(), base)


def check_void_entries(eng, to_tensor):
    """boxes_suite.check_void_entries for the tiles call: a void entry in the middle and one entry per violated clause of the validity rule, B = 2 with both
    valid tiles in image 1; nothing is written outside the outputs; on image 1 the call equals the one whose bad entries are the whole frame of image 0
    (the same model batch); image 0, without a valid tile, is the base."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    from comfyui_sdmatte_amd.engine import _ptr
    image, trimap = BS.frames(2, seed=23)
    good = [[1, 10, 20, 48, 48], [1, 40, 50, 48, 48]]                                            # overlapping
    entries = [good[0]] + [list(e) for e in BS.BAD_ENTRIES] + [good[1]]
    tiles = tiles_tensor(entries)
    assert len(entries) == 13
    same_batch = tiles_tensor([good[0]] + [[0, 0, 0, H_E2E, W_E2E]] * len(BS.BAD_ENTRIES) + [good[1]])
    img, tri, lst = to_tensor(image), to_tensor(trimap), to_tensor(tiles)
    px, guard = trimap.numel(), 4096
    abuf, mbuf = torch.full((px + 2 * guard, ), -7.0, device=img.device), torch.full((px * 4 + 2 * guard, ), -7.0, device=img.device)
    rc = eng.lib.sdm_apply_matte_tiles(eng.h, _ptr(img), _ptr(tri), 2, H_E2E, W_E2E, S_E2E, 0, _ptr(lst), lst.shape[0], 6, None, 1, 1, ctypes.c_double(C_E2E),
                                       _ptr(abuf[guard:]), _ptr(mbuf[guard:]), eng._kind(img), None)
    eng.synchronize()
    assert rc == 0
    for buf, n in ((abuf, px), (mbuf, 4 * px)):
        assert bool((buf[:guard] == -7).all()) and bool((buf[guard + n:] == -7).all())
    a, m = abuf[guard:guard + px].view(2, H_E2E, W_E2E), mbuf[guard:guard + 4 * px].view(2, H_E2E, W_E2E, 4)
    a2, m2 = call(eng, to_tensor, image, trimap, same_batch, "matted_rgba", True, 6)
    assert torch.equal(a[1], a2[1]) and torch.equal(m[1], m2[1])
    want0, _ = N.refine_and_compose(definite(trimap[:1]), image[:1], trimap[:1], "matted_rgba", True, C_E2E)
    assert torch.equal(a[0].cpu(), want0[0]) and not torch.equal(a2[0].cpu(), want0[0])
    a0, _ = call(eng, to_tensor, image, trimap, tiles_tensor([VOID]))                             # no valid entry at all
    assert torch.equal(a0.cpu(), definite(trimap))


def check_call_errors(eng, to_tensor):
    """N = -1, N = 17, a bad feather_px, output_mode, S or plane size are SDM_ERR_INVALID with a message that names the argument; Python raises; outputs
    pre-filled with -7 stay untouched."""
    import pytest
    from comfyui_sdmatte_amd.engine import _ptr
    image, trimap = BS.frames(1)
    image, trimap = to_tensor(image), to_tensor(trimap)
    ok = to_tensor(tiles_tensor([[0, 10, 20, 48, 48]]))
    with pytest.raises(IndexError):
        eng.apply_matte_tiles(image, trimap[:, :50, :70], ok, S_E2E, False, "alpha_only", False, C_E2E)
    for bad in ((image, trimap[0], ok, "alpha_only", {}), (image, trimap, ok, "nope", {}), (image, trimap, ok.repeat(17, 1), "alpha_only", {}),
                (image, trimap, ok.float(), "alpha_only", {}), (image, trimap, ok[:, :4], "alpha_only", {}), (image[..., :2], trimap, ok, "alpha_only", {}),
                (image, trimap, ok, "alpha_only", dict(feather_px=-1)), (image, trimap, ok, "alpha_only", dict(feather_px=1025)),
                (image, trimap, ok, "alpha_only", dict(feather_px=1.5)), (image, trimap, ok, "alpha_only", dict(base=trimap[:, :50]))):
        with pytest.raises(ValueError):
            eng.apply_matte_tiles(bad[0], bad[1], bad[2], S_E2E, False, bad[3], False, C_E2E, **bad[4])
    B, H, W = trimap.shape
    alpha, matted = torch.full_like(trimap, -7.0), torch.full_like(image, -7.0)
    lst = to_tensor(tiles_tensor([[0, 10, 20, 48, 48]] * 17))
    kind = eng._kind(image)

    def raw(N=1, mode=0, S=S_E2E, H_=H, feather=0, tiles=lst):
        return eng.lib.sdm_apply_matte_tiles(eng.h, _ptr(image), _ptr(trimap), B, H_, W, S, 0, _ptr(tiles), N, feather, None, mode, 0, ctypes.c_double(C_E2E),
                                             _ptr(alpha), _ptr(matted), kind, None)
    assert raw(N=-1) == -1 and b"N = -1" in eng.lib.sdm_last_error(eng.h)
    assert raw(N=17) == -1 and b"N = 17" in eng.lib.sdm_last_error(eng.h)
    assert raw(tiles=None) == -1 and b"tiles_n5" in eng.lib.sdm_last_error(eng.h)
    assert raw(feather=-1) == -1 and b"feather_px = -1" in eng.lib.sdm_last_error(eng.h)
    assert raw(feather=1025) == -1 and b"feather_px = 1025" in eng.lib.sdm_last_error(eng.h)
    assert raw(mode=3) == -1 and b"output mode" in eng.lib.sdm_last_error(eng.h)
    assert raw(mode=-1) == -1
    assert raw(S=65) == -1 and b"multiple of 64" in eng.lib.sdm_last_error(eng.h)
    assert raw(H_=0) == -1 and b"bad plane size" in eng.lib.sdm_last_error(eng.h)
    eng.synchronize()
    assert bool((alpha == -7).all()) and bool((matted == -7).all())
