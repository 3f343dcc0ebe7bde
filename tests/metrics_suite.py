"""Cases, references and the tolerance rule of sdm_matte_metrics (include/sdmatte.h), shared by tests/test_emu_metrics.py (fiber emulator),
tests/test_gpu_metrics.py (MI355X) and tests/test_node_metrics_cpu.py (torch restatement).

Two references written independently of each other and of the kernels:
  * `loop_reference`: numpy fp64 straight from the definition - flood-fill labelling, the explicit 2-D kernel G (x) D on an edge-padded array;
  * `sdmatte_nodes.matte_metrics` on fp64 tensors: the vectorised torch restatement (separable filter, label equivalence).
They must agree on every case (levels exactly, sums to 1e-12 relative): `check_references_agree`.

Exact on every implementation: n, max|e|, the level map.  The six sums, per case and per sum:
    |got - ref64| <= max(4 d32, 2^-20 max(1, |ref64|))
d32 = the larger distance to ref64 of two fp32 variants computed HERE, never from the code under test: the torch restatement on fp32 tensors and
`variant32` (numpy fp32, terms by a separable filter of its own, rows added one after the other).  The rule is that of harmonize_suite.tolerance, taken
relative because these are sums and not values in [0, 1]."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUM_SLOTS = (1, 2, 3, 4, 6, 7)
EXACT_SLOTS = (0, 5)
SLOT_NAMES = ("n", "sad", "sse", "grad", "conn", "max", "sad_frame", "sse_frame")
F32 = np.float32


def _nodes():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    load_package()
    from comfyui_sdmatte_amd import sdmatte_nodes
    return sdmatte_nodes


# ---- the definition, in plain loops -------------------------------------------------------------------------------------------------------
def weights(sigma):
    """(r, G, D) as the header defines them: double from the fp32 sigma, G (x) D of unit L2 norm, rounded to fp32."""
    s = float(F32(sigma))
    r = int(np.ceil(s * np.sqrt(-2.0 * np.log(np.sqrt(2.0 * np.pi) * s * 0.01))))
    G = [np.exp(-(i * i) / (2.0 * s * s)) / (s * np.sqrt(2.0 * np.pi)) for i in range(-r, r + 1)]
    D = [-i * G[i + r] / (s * s) for i in range(-r, r + 1)]
    norm = np.sqrt(np.sqrt(sum(v * v for v in G) * sum(v * v for v in D)))
    return r, np.array([v / norm for v in G]).astype(F32), np.array([v / norm for v in D]).astype(F32)


def sanitise(a, dtype):
    a = np.asarray(a, dtype).copy()
    a[np.isnan(a)] = 0.0
    return np.clip(a, 0.0, 1.0)


def region_of(trimap, shape):
    if trimap is None:
        return np.ones(shape, bool)
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(trimap, F32) - F32(0.5)) < F32(0.25)      # one fp32 subtraction, fabsf, one compare: NaN is outside


def _flood_components(cls):
    """4-connected components of a bool [H,W] by flood fill: a list of (smallest pixel index, list of pixel indices)."""
    H, W = cls.shape
    seen = np.zeros((H, W), bool)
    comps = []
    for y in range(H):
        for x in range(W):
            if not cls[y, x] or seen[y, x]:
                continue
            stack, pix = [(y, x)], []
            seen[y, x] = True
            while stack:
                cy, cx = stack.pop()
                pix.append(cy * W + cx)
                for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                    if 0 <= ny < H and 0 <= nx < W and cls[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        stack.append((ny, nx))
            comps.append((min(pix), pix))
    return comps


def loop_levels(c):
    """c = min(p, g) [H,W] fp32-valued -> (L int32 [H,W], omegas: list of 10 bool [H,W]).  The scan meets components in the order of their smallest
    pixel, so `>` keeps the first of the largest."""
    H, W = c.shape
    L = np.zeros((H, W), np.int32)
    omegas = []
    for k in range(1, 11):
        t = F32(k) / F32(10.0)
        best = None
        for first, pix in _flood_components(np.asarray(c, F32) >= t):
            if best is None or len(pix) > len(best[1]):
                best = (first, pix)
        om = np.zeros(H * W, bool)
        if best is not None:
            om[best[1]] = True
        om = om.reshape(H, W)
        omegas.append(om)
        L[(L == k - 1) & om] = k
    return L, omegas


def loop_reference(pred, gt, trimap, sigma, conn):
    """-> (raw float64 [B,8], levels int32 [B,H,W] or None, omegas per image or None)."""
    B, H, W = pred.shape
    r, G, D = weights(sigma)
    Kx = np.outer(G.astype(np.float64), D.astype(np.float64))      # [i (rows), j (columns)]: a_x = sum_ij G_i D_j a(y + i, x + j)
    Ky = np.outer(D.astype(np.float64), G.astype(np.float64))
    p, g = sanitise(pred, np.float64), sanitise(gt, np.float64)
    reg = region_of(trimap, pred.shape)
    raw = np.zeros((B, 8))
    levels = np.zeros((B, H, W), np.int32) if conn else None
    omegas = [] if conn else None
    theta = float(F32(0.15))
    for b in range(B):
        pp, gp = np.pad(p[b], r, mode="edge"), np.pad(g[b], r, mode="edge")
        if conn:
            levels[b], om = loop_levels(np.minimum(sanitise(pred[b], F32), sanitise(gt[b], F32)))
            omegas.append(om)
        for y in range(H):
            for x in range(W):
                e = p[b, y, x] - g[b, y, x]
                raw[b, 6] += abs(e)
                raw[b, 7] += e * e
                if not reg[b, y, x]:
                    continue
                wp, wg = pp[y:y + 2 * r + 1, x:x + 2 * r + 1], gp[y:y + 2 * r + 1, x:x + 2 * r + 1]
                mp = np.sqrt((Kx * wp).sum() ** 2 + (Ky * wp).sum() ** 2)
                mg = np.sqrt((Kx * wg).sum() ** 2 + (Ky * wg).sum() ** 2)
                raw[b, 0] += 1
                raw[b, 1] += abs(e)
                raw[b, 2] += e * e
                raw[b, 3] += (mp - mg) ** 2
                raw[b, 5] = max(raw[b, 5], abs(e))
                if conn:
                    l = float(F32(levels[b, y, x]) / F32(10.0))
                    dp, dg = p[b, y, x] - l, g[b, y, x] - l
                    raw[b, 4] += abs((1.0 - (dp if dp >= theta else 0.0)) - (1.0 - (dg if dg >= theta else 0.0)))
    return raw, levels, omegas


def variant32(pred, gt, trimap, sigma, conn, levels):
    """raw [B,8] in numpy fp32 (returned as float64): every term in fp32 by a separable filter written here, every sum row by row, the rows one after
    the other.  `levels` is the exact level map (the references')."""
    B, H, W = pred.shape
    r, G, D = weights(sigma)
    p, g = sanitise(pred, F32), sanitise(gt, F32)
    reg = region_of(trimap, pred.shape)

    def mag(a):
        pad = np.pad(a, ((0, 0), (r, r), (r, r)), mode="edge")
        vg, vd = np.zeros((B, H, W + 2 * r), F32), np.zeros((B, H, W + 2 * r), F32)
        for k in range(2 * r + 1):
            vg = vg + G[k] * pad[:, k:k + H]
            vd = vd + D[k] * pad[:, k:k + H]
        ax, ay = np.zeros((B, H, W), F32), np.zeros((B, H, W), F32)
        for k in range(2 * r + 1):
            ax = ax + D[k] * vg[:, :, k:k + W]
            ay = ay + G[k] * vd[:, :, k:k + W]
        return np.sqrt(ax * ax + ay * ay)

    def rows(t):
        out = np.zeros(B, F32)
        for y in range(H):
            out = out + t[:, y].sum(axis=1, dtype=F32)
        return out.astype(np.float64)
    e = p - g
    ae, ee = np.abs(e), e * e
    dm = mag(p) - mag(g)
    zero = F32(0.0)
    raw = np.zeros((B, 8))
    raw[:, 0] = reg.reshape(B, -1).sum(1)
    raw[:, 1], raw[:, 2], raw[:, 3] = rows(np.where(reg, ae, zero)), rows(np.where(reg, ee, zero)), rows(np.where(reg, dm * dm, zero))
    raw[:, 5] = np.where(reg, ae, zero).reshape(B, -1).max(1)
    raw[:, 6], raw[:, 7] = rows(ae), rows(ee)
    if conn:
        l = levels.astype(F32) / F32(10.0)
        phi = lambda a: F32(1.0) - np.where(a - l >= F32(0.15), a - l, zero)
        raw[:, 4] = rows(np.where(reg, np.abs(phi(p) - phi(g)), zero))
    return raw


# ---- the case list --------------------------------------------------------------------------------------------------------------------------
def _smooth(rng, B, H, W, passes=6):
    t = rng.uniform(-1.0, 1.0, (B, H, W))
    for _ in range(passes):
        t = (t + np.roll(t, 1, 1) + np.roll(t, -1, 1) + np.roll(t, 1, 2) + np.roll(t, -1, 2)) / 5.0
    return t / np.abs(t).max()


def _soft_gt(rng, B, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((B, H, W))
    for b in range(B):
        cy, cx, ry, rx = H * (0.45 + 0.1 * b), W * (0.5 - 0.06 * b), H * 0.33, W * 0.3
        d = np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)
        out[b] = np.clip((1.15 - d) / 0.45, 0.0, 1.0)
    return out


def _band_trimap(gt):
    tri = np.where(gt >= 0.98, 1.0, np.where(gt <= 0.02, 0.0, 0.5))
    grow = tri == 0.5
    for ax in (1, 2):                                                   # the band, two pixels wider (no wrap-around: the frame's border is certain)
        for sh in (1, 2, -1, -2):
            grow = grow | np.roll(tri == 0.5, sh, ax)
    grow[:, :2], grow[:, -2:], grow[:, :, :2], grow[:, :, -2:] = False, False, False, False
    return np.where(grow, 0.5, tri)


def _generic(seed, B, H, W, peak=1.0):
    rng = np.random.default_rng(seed)
    gt = _soft_gt(rng, B, H, W) * peak
    pred = np.clip(gt + 0.08 * _smooth(rng, B, H, W), 0.0, 1.0)
    return pred.astype(F32), gt.astype(F32), _band_trimap(gt / peak).astype(F32)


def _seams():
    """1 x 65 x 130: a one-pixel snake (rows 2, 10, ..., 58 and the last row 64, joined at alternating ends) that crosses the 64-pixel tile seams in both
    directions, and a 5 x 5 blob between two of its rows."""
    H, W = 65, 130
    gt = np.zeros((1, H, W), F32)
    rows = list(range(2, 60, 8)) + [64]
    for n, y in enumerate(rows):
        gt[0, y, 1:W - 1] = 0.95
        if n + 1 < len(rows):
            x = W - 2 if n % 2 == 0 else 1
            gt[0, y:rows[n + 1] + 1, x] = 0.95
    gt[0, 4:9, 20:25] = 0.95
    pred = (gt * F32(0.97)).astype(F32)
    return pred, gt, None


def _tie():
    """1 x 40 x 120: two 6 x 6 blobs of one value in different tiles; the one further right starts two rows higher, so it holds the smaller index."""
    gt = np.zeros((1, 40, 120), F32)
    gt[0, 10:16, 100:106] = 0.85
    gt[0, 12:18, 5:11] = 0.85
    pred = (gt * F32(0.9) + F32(0.1)).astype(F32)                       # above gt everywhere: min(p, g) = g
    return pred, gt, None


def _not_nested():
    """1 x 40 x 70: blob A (10 x 10 at 0.45) is the largest component up to level 4, blob B (5 x 5, pred 0.75, gt 0.95) from level 5 on, so B's pixels are
    frozen at level 0.  With l = 0 their Conn term is |0.75 - 0.95| = 0.2; an implementation that lets them follow the later Omegas gives them l = 0.7 and
    the term 0.25 (phi(p) = 1, phi(g) = 0.75): the Conn sum moves by 1.25 (check_case_properties asserts it)."""
    gt = np.zeros((1, 40, 70), F32)
    gt[0, 5:15, 5:15] = 0.45
    gt[0, 25:30, 50:55] = 0.95
    pred = gt.copy()
    pred[0, 5:15, 5:15] = 0.5
    pred[0, 25:30, 50:55] = 0.75
    return pred, gt, None


def _empty_levels():
    pred, gt, tri = _generic(11, 1, 40, 70, peak=0.55)
    pred = np.maximum(pred, gt * F32(1.0)).astype(F32)                  # min(p, g) = g, whose largest value is fp32(0.55)
    return pred, gt, tri


def _dirty():
    pred, gt, tri = _generic(5, 2, 33, 70)
    pred, tri = pred.copy(), tri.copy()
    pred[0, 10, 20:24] = np.nan
    pred[0, 12, 30:34] = -1.0
    pred[1, 15, 30:40] = 2.0
    tri[0, 16, 25:45] = np.nan
    tri[1, 10:12, 30:40] = np.nan
    return pred, gt, tri


def _border(H=15, W=12):
    gt = np.ones((1, H, W), F32)
    gt[0, :, 0] = 0.0
    gt[0, -1, :] = 0.0
    pred = np.ones((1, H, W), F32)
    pred[0, :, 0] = 0.25
    pred[0, :, 1] = 0.75
    pred[0, -1, :] = 0.125
    pred[0, -2, :] = 0.875
    return pred, gt, None


@functools.lru_cache(maxsize=None)
def cases():
    """(name, pred, gt, trimap or None, grad_sigma, conn) - fp32 arrays [B,H,W]."""
    g = _generic(3, 2, 70, 133)
    ident = _generic(9, 1, 37, 70)
    out = [("generic_2x70x133", *g, 1.4, True),
           ("generic_no_conn", *g, 1.4, False),
           ("seams_65x130", *_seams(), 1.4, True),
           ("tie_40x120", *_tie(), 1.4, True),
           ("not_nested_40x70", *_not_nested(), 1.4, True),
           ("empty_levels_40x70", *_empty_levels(), 1.4, True),
           ("identity_37x70", ident[1], ident[1], ident[2], 1.4, True),
           ("empty_region_37x70", ident[0], ident[1], np.zeros_like(ident[2]), 1.4, True),
           ("dirty_2x33x70", *_dirty(), 2.0, True),
           ("border_s0.25", *_border(), 0.25, False),
           ("border_s1.4", *_border(), 1.4, True),
           ("border_s4", *_border(), 4.0, False)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def batch_of_three():
    """(pred, gt, trimap) [3,70,133]: three different images, for "an image alone and as part of a batch"."""
    a, b = _generic(3, 2, 70, 133), _generic(21, 1, 70, 133)
    return tuple(np.ascontiguousarray(np.concatenate([x[:1], y, x[1:]])) for x, y in zip(a, b))


def case(name):
    return next(c for c in cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def references(name):
    """-> (raw64 [B,8], levels or None, d32 [B,8], omegas or None) of a case, computed once."""
    _, pred, gt, tri, sigma, conn = case(name)
    raw64, levels, omegas = loop_reference(pred, gt, tri, sigma, conn)
    N = _nodes()
    t32 = N.matte_metrics(torch.from_numpy(pred), torch.from_numpy(gt), None if tri is None else torch.from_numpy(tri), sigma, conn)["raw"].numpy()
    v32 = variant32(pred, gt, tri, sigma, conn, levels)
    d32 = np.maximum(np.abs(t32 - raw64), np.abs(v32 - raw64))
    for a in (raw64, d32):
        a.setflags(write=False)
    return raw64, levels, d32, omegas


def tolerance(d32, ref):
    return max(4.0 * d32, 2.0 ** -20 * max(1.0, abs(ref)))


def compare(name, raw, levels, report=None):
    """raw [B,8] float64 and levels (or None) of an implementation against the references of case `name`; returns the largest d / d32 seen."""
    raw64, lev64, d32, _ = references(name)
    raw = np.asarray(raw.detach().cpu().numpy() if hasattr(raw, "detach") else raw, np.float64)
    assert raw.shape == raw64.shape and np.isfinite(raw).all(), (name, raw.shape)
    for s in EXACT_SLOTS:
        assert np.array_equal(raw[:, s], raw64[:, s].astype(F32).astype(np.float64) if s == 5 else raw64[:, s]), (name, SLOT_NAMES[s], raw[:, s], raw64[:, s])
    if lev64 is None:
        assert levels is None and np.all(raw[:, 4] == 0.0), name
    elif levels is not None:
        got = levels.detach().cpu().numpy() if hasattr(levels, "detach") else np.asarray(levels)
        assert got.dtype == np.int32 and np.array_equal(got, lev64), (name, int((got != lev64).sum()))
    worst = 0.0
    for b in range(raw.shape[0]):
        for s in SUM_SLOTS:
            d, tol = abs(raw[b, s] - raw64[b, s]), tolerance(d32[b, s], raw64[b, s])
            ratio = d / max(d32[b, s], 1e-300) if d > 0 else 0.0
            line = f"[metrics] {name} image {b} {SLOT_NAMES[s]}: ref = {raw64[b, s]:.9e} d32 = {d32[b, s]:.3e} tol = {tol:.3e} d = {d:.3e} ratio = {ratio:.2f}"
            print(line)
            if report is not None:
                report.append(line)
            assert d <= tol, line
            if d32[b, s] > 0:
                worst = max(worst, ratio)
    return worst


def check(metrics, to_tensor, report=None):
    """metrics(pred, gt, trimap or None, grad_sigma, conn, return_levels) -> the dict of Engine.matte_metrics, on tensors made by `to_tensor`; every case.
    The level map is asked for and compared on every Conn case."""
    worst = 0.0
    for name, pred, gt, tri, sigma, conn in cases():
        res = metrics(*(None if t is None else to_tensor(torch.from_numpy(t)) for t in (pred, gt, tri)), sigma, conn, conn)
        assert not conn or res.get("levels") is not None, name
        worst = max(worst, compare(name, res["raw"], res.get("levels"), report))
    print(f"[metrics] largest d / d32 over the case list: {worst:.2f}")
    return worst


def launches(with_conn, level_given=False):
    """the launches of one call (include/sdmatte.h): a function of with_conn (and, by contract, of level_given: mm_conn writes the map, so it is the same)"""
    del level_given
    out = {"mm_pixel": 1, "mm_finalize": 1}
    if with_conn:
        out.update({"cc_tile": 10, "cc_seam": 10, "cc_flatten": 10, "cc_select": 20, "mm_level": 10, "mm_conn": 1})
    return out


def expected_counts(calls):
    """calls: iterable of (with_conn, level_given)"""
    out = {}
    for c in calls:
        for k, v in launches(*c).items():
            out[k] = out.get(k, 0) + v
    return out


def case_calls():
    """(with_conn, level_given) of the calls `check` makes"""
    return [(c[5], c[5]) for c in cases()]


# ---- what the cases are for (asserted on the reference, so that none passes vacuously) --------------------------------------------------------
def check_case_properties():
    raw, lev, _, om = references("seams_65x130")
    big = om[0][0]                                                     # Omega_1 of the one image
    tiles = {(y // 64, x // 64) for y, x in zip(*np.nonzero(big))}
    assert len(tiles) >= 3 and {t[0] for t in tiles} == {0, 1} and {t[1] for t in tiles} == {0, 1, 2}, tiles
    assert lev[0, 5, 22] == 0 and lev[0, 2, 5] == 9 and lev[0, 64, 100] == 9          # the blob loses, the snake is one component down to the last row
    raw, lev, _, om = references("tie_40x120")
    assert lev[0, 10, 100] == 8 and lev[0, 12, 5] == 0 and set(np.unique(lev)) == {0, 8}      # equal areas: the smaller pixel index wins
    raw, lev, _, om = references("not_nested_40x70")
    later = [k for k in range(2, 11) if (om[0][k - 1] & (lev[0] < k - 1)).any()]
    assert later and lev[0, 27, 52] == 0 and lev[0, 10, 10] == 4, later               # a later Omega holds frozen pixels, and they stay frozen
    # ... and the Conn sum sees a level map without the freeze (L = the number of Omegas a pixel lies in up to its first gap ignored: B follows Omega_5..7)
    _, pred, gt, tri, sigma, _ = case("not_nested_40x70")
    thawed = lev.copy()
    for k in range(1, 11):
        thawed[0][om[0][k - 1] & (thawed[0] < k)] = k
    assert thawed[0, 27, 52] == 7 and np.array_equal(thawed[0, 5:15, 5:15], lev[0, 5:15, 5:15])
    moved = abs(variant32(pred, gt, tri, sigma, True, thawed)[0, 4] - raw[0, 4])
    assert moved > 1.0 and moved > 1e4 * tolerance(references("not_nested_40x70")[2][0, 4], raw[0, 4]), moved
    raw, lev, _, om = references("empty_levels_40x70")
    _, pred, gt, _, _, _ = case("empty_levels_40x70")
    assert float(np.minimum(pred, gt).max()) == float(F32(0.55)) and lev.max() == 5 and not om[0][5].any()
    raw, lev, _, _ = references("identity_37x70")
    assert raw[0, 0] > 100 and np.all(raw[0, [1, 2, 3, 4, 5, 6, 7]] == 0.0)
    raw, _, _, _ = references("empty_region_37x70")
    assert np.all(raw[0, :6] == 0.0) and raw[0, 6] > 0 and raw[0, 7] > 0
    _, pred, gt, tri, _, _ = case("dirty_2x33x70")
    assert np.isnan(pred).sum() == 4 and np.isnan(tri).sum() == 40 and not region_of(tri, tri.shape)[np.isnan(tri)].any()
    for s, r in ((0.25, 1), (1.4, 4), (4.0, 9)):
        assert weights(s)[0] == r
    assert case("border_s4")[1].shape[2] < 2 * 9 + 1
    raw, _, _, _ = references("generic_2x70x133")
    assert np.all(raw[:, 0] > 500) and np.all(raw[:, 1:5] > 0)


def check_references_agree():
    """loop_reference against the torch restatement in fp64 on every case: levels exactly, sums to 1e-12 relative."""
    N = _nodes()
    for name, pred, gt, tri, sigma, conn in cases():
        raw64, lev64, _, _ = references(name)
        res = N.matte_metrics(torch.from_numpy(pred).double(), torch.from_numpy(gt).double(), None if tri is None else torch.from_numpy(tri).double(),
                              sigma, conn, return_levels=conn)
        got = res["raw"].numpy()
        if conn:
            assert res["levels"].dtype == torch.int32 and np.array_equal(res["levels"].numpy(), lev64), name
        assert np.array_equal(got[:, [0, 5]], raw64[:, [0, 5]]), name
        err = np.abs(got - raw64)
        assert np.all(err <= 1e-12 * np.abs(raw64)), (name, err.max(), got, raw64)
