"""Shared by tests/test_node_cleanmask_cpu.py, tests/test_emu_cleanmask.py and tests/test_gpu_cleanmask.py: the mask clean-up cases and a reference
that shares no code with the kernels (csrc/k_cclabel.h) or with the CPU restatement (sdmatte_nodes.clean_mask): row runs, joined between
neighbouring rows by a dictionary union-find.  Every comparison is exact, on the bit patterns (a NaN that is copied stays the same NaN)."""
import functools

import numpy as np
import torch

T = 64      # SDM_CC_T, the tile side of the labelling kernels


# ---- reference ----------------------------------------------------------------------------------------------------------------------------
def _runs(row):
    """[(x0, x1)] half-open runs of True in a 1-D bool array."""
    d = np.diff(np.concatenate(([0], row.astype(np.int8), [0])))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def components(cls, diagonal):
    """cls bool [H,W] -> list of components, each a list of runs (y, x0, x1), ordered by their smallest pixel index y*W + x.  diagonal: 8-connected."""
    H, _ = cls.shape
    parent = {}

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    reach = 1 if diagonal else 0
    prev = []
    for y in range(H):
        cur = [(y, x0, x1) for x0, x1 in _runs(cls[y])]
        for r in cur:
            parent[r] = r
        i = 0
        for r in cur:
            while i < len(prev) and prev[i][2] + reach <= r[1]:          # ends left of r: left of every later run too
                i += 1
            j = i
            while j < len(prev) and prev[j][1] < r[2] + reach:
                a, b = find(prev[j]), find(r)
                if a != b:
                    parent[max(a, b)] = min(a, b)                        # tuples order like pixel indices: the root is the first run
                j += 1
        prev = cur
    groups = {}
    for r in sorted(parent):
        groups.setdefault(find(r), []).append(r)
    return [groups[k] for k in sorted(groups)]


def reference(mask, threshold=0.5, min_area=64, keep_largest=False, max_hole_area=64, binarize=False):
    """(out fp32 [B,H,W], stats int32 [B,4]) by the definition in include/sdmatte.h."""
    mask = np.asarray(mask, np.float32)
    B, H, W = mask.shape
    out = mask.copy()
    stats = np.zeros((B, 4), np.int32)
    for b in range(B):
        with np.errstate(invalid="ignore"):
            fg = mask[b] > np.float32(threshold)
        comps = components(fg, True)
        areas = [sum(x1 - x0 for _, x0, x1 in c) for c in comps]
        stats[b, 0] = len(comps)
        keep = np.zeros_like(fg)
        if min_area > 1 or keep_largest:
            best = areas.index(max(areas)) if comps else -1              # index(): the first of equal areas = smallest pixel index
            for i, c in enumerate(comps):
                if areas[i] >= min_area and (not keep_largest or i == best):
                    for y, x0, x1 in c:
                        keep[y, x0:x1] = True
                else:
                    stats[b, 1] += 1
        else:
            keep = fg.copy()
        filled = np.zeros_like(fg)
        if max_hole_area > 0:
            for c in components(~keep, False):
                if any(y == 0 or y == H - 1 or x0 == 0 or x1 == W for y, x0, x1 in c):
                    continue
                if sum(x1 - x0 for _, x0, x1 in c) <= max_hole_area:
                    stats[b, 2] += 1
                    for y, x0, x1 in c:
                        filled[y, x0:x1] = True
        removed = fg & ~keep
        if binarize:
            out[b] = fg.astype(np.float32)
        out[b][removed] = 0.0
        out[b][filled] = 1.0
        stats[b, 3] = int(removed.sum()) + int(filled.sum())
    return out, stats


# ---- masks ----------------------------------------------------------------------------------------------------------------------------------
def blobs(seed, B, H, W, n=6):
    """Soft random blobs in [0, 1] (a few Gaussian bumps per image, different per image) with speckle: single pixels and 2x2 dots switched on and off."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.zeros((B, H, W), np.float32)
    for b in range(B):
        for _ in range(n):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            s = rng.uniform(0.04, 0.2) * max(H, W)
            out[b] = np.maximum(out[b], np.exp(-((ys - cy) ** 2 + (xs - cx) ** 2) / (2 * s * s)).astype(np.float32))
        for _ in range(max(4, H * W // 400)):
            y, x, k = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(1, 3))
            out[b, y:y + k, x:x + k] = np.float32(rng.uniform(0.6, 1.0)) if out[b, y, x] <= 0.5 else np.float32(rng.uniform(0.0, 0.4))
    return out


def _empty(B, H, W):
    return np.zeros((B, H, W), np.float32)


def _full(B, H, W):
    return np.ones((B, H, W), np.float32)


def _nan_sprinkled(B, H, W):
    m = blobs(H * 7 + W, B, H, W, n=3)
    m[:, ::3, ::5] = np.nan
    m[:, 1::4, 2::3] = np.float32(0.5)                                   # exactly the default threshold: background
    return m


def _corners(B, H, W):
    m = _empty(B, H, W)
    m[:, 0, 0] = m[:, 0, W - 1] = m[:, H - 1, 0] = m[:, H - 1, W - 1] = 1.0
    return m


def _checkerboard(B, H, W):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.broadcast_to(((ys + xs) % 2 == 0).astype(np.float32), (B, H, W)).copy()


def _rings(B, H, W):
    """Concentric one-pixel rectangles, two pixels apart, centred differently per image."""
    ys, xs = np.mgrid[0:H, 0:W]
    m = _empty(B, H, W)
    for b in range(B):
        d = np.maximum(np.abs(ys - (H // 2 + 3 * b)), np.abs(xs - (W // 2 - 5 * b)))
        m[b] = ((d % 2 == 1) & (d < 40)).astype(np.float32)
    return m


def _spiral(B, H, W):
    """A one-pixel-wide rectangular spiral from the top left corner inwards, its arms one pixel apart: a walk that turns right whenever the pixel after
    the next one is already part of it."""
    g = np.zeros((H, W), bool)
    y, x, dy, dx, turns = 0, 0, 0, 1, 0
    g[0, 0] = True
    while turns < 2:
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if 0 <= ny < H and 0 <= nx < W and not g[ny, nx] and not (0 <= ay < H and 0 <= ax < W and g[ay, ax]):
            y, x, turns = ny, nx, 0
            g[y, x] = True
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return np.broadcast_to(g.astype(np.float32), (B, H, W)).copy()


def _serpentine(B, H, W):
    """One-pixel rows every second row, joined alternately at the right and the left end: a single line through the whole image."""
    m = _empty(B, H, W)
    m[:, ::2, :] = 1.0
    for i, y in enumerate(range(1, H, 2)):
        m[:, y, W - 1 if i % 2 == 0 else 0] = 1.0
    return m


def _comb(B, H, W):
    m = _empty(B, H, W)
    m[:, H - 1, :] = 1.0
    m[:, H // 4:, ::2] = 1.0                                              # teeth one pixel wide, one pixel apart: the gaps are open at the top
    m[:, 0, ::3] = 1.0                                                    # loose pixels above them
    return m


def _staircase(B, H, W):
    """A diagonal, one pixel per row: one 8-connected component that separates nothing for the 4-connected background; plus a closed box around a
    second diagonal, whose two halves are two holes."""
    m = _empty(B, H, W)
    for i in range(min(H, W)):
        m[:, i, i] = 1.0
    s = min(H, W, 12)
    if s >= 5:
        y0, x0 = H - s, 0
        m[:, y0, x0:x0 + s] = m[:, y0 + s - 1, x0:x0 + s] = 1.0
        m[:, y0:y0 + s, x0] = m[:, y0:y0 + s, x0 + s - 1] = 1.0
        for i in range(s):
            m[:, y0 + i, x0 + i] = 1.0
    return m


def _batch_pair(B, H, W):
    """Bottom row of image b and top row of image b + 1, at column 0 and at column W - 1: four components per inner image, never one."""
    m = _empty(B, H, W)
    m[:, H - 1, 0] = m[:, H - 1, W - 1] = 1.0
    m[:, 0, 0] = m[:, 0, W - 1] = 1.0
    m[:, H // 2, : max(1, W // 2)] = 1.0                                  # the largest component of every image
    return m


def _tie(B, H, W):
    """Two components of the same, largest area (and a smaller one): keep_largest takes the one with the smallest pixel index."""
    m = _empty(B, H, W)
    if W >= H:
        k = max(1, W // 5)
        m[:, H - 1, :k] = 1.0
        m[:, 0, W - k:] = 1.0
        m[:, H // 2, W // 2: W // 2 + max(1, k - 1)] = 1.0 if H > 2 and k > 1 else 0.0
    else:
        k = max(1, H // 5)
        m[:, :k, W - 1] = 1.0
        m[:, H - k:, 0] = 1.0
    return m


PATTERNS = [("empty", _empty), ("full", _full), ("nan", _nan_sprinkled), ("corners", _corners), ("checkerboard", _checkerboard), ("rings", _rings),
            ("spiral", _spiral), ("serpentine", _serpentine), ("comb", _comb), ("staircase", _staircase), ("batch_pair", _batch_pair), ("tie", _tie),
            ("blobs", lambda B, H, W: blobs(H * 1000 + W, B, H, W))]
BATCHED = {"rings", "batch_pair", "blobs", "nan"}                         # B = 3
SHAPES = [(1, 1), (1, 300), (300, 1), (T + 1, T - 1), (2 * T + 2, T + 6), (257, 515)]

ONE = float(np.nextafter(np.float32(1), np.float32(0)))
# (threshold, min_area, keep_largest, max_hole_area, binarize)
BOTH = (0.5, 6, False, 5, False)
PARAMS = [
    (0.5, 0, False, 0, False),            # all stages off: identity
    (0.5, 1, False, 0, True),             # ... binarised
    (0.5, 6, False, 0, True),             # A only
    (0.5, 0, False, 5, False),            # B only
    (0.5, 64, False, 64, True),           # both, the node's defaults
    (0.5, 0, True, 0, False),             # largest only
    (0.5, 3, True, 2000, False),          # largest, then its holes (the other components' pixels enlarge them)
    (0.5, 1 << 28, True, 0, False),       # larger than anything: empty
    (0.0, 3, False, 3, False),
    (ONE, 2, False, 2, True),
]
SPECIAL = {"checkerboard": [(0.5, 0, False, 1, False), (0.5, 0, False, 0, True)], "tie": [(0.5, 0, True, 0, False), (0.5, 2, True, 9, True)]}


@functools.lru_cache(maxsize=None)
def cases():
    """((name, mask fp32 [B,H,W], params, expected out, expected stats), ...): every pattern at every shape with BOTH and one more parameter set (in
    rotation; the checkerboard and the tie with their own).  The reference runs once per process."""
    out, k = [], 0
    for H, W in SHAPES:
        for pname, fn in PATTERNS:
            mask = fn(3 if pname in BATCHED else 1, H, W)
            mask.setflags(write=False)
            more = SPECIAL.get(pname)
            if more is None:
                more = [PARAMS[k % len(PARAMS)]]
                k += 1
            for p in [BOTH] + more:
                want, stats = reference(mask, *p)
                want.setflags(write=False); stats.setflags(write=False)
                out.append((f"{pname}_{H}x{W}_{p}", mask, p, want, stats))
    return tuple(out)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_clean_mask(fn, to_device, select=None):
    """fn(mask tensor, threshold, min_area, keep_largest, max_hole_area, binarize) -> (out tensor, stats tensor); every case equals the reference."""
    for name, mask, p, want, wstats in cases():
        if select is not None and not select(name):
            continue
        got, stats = fn(to_device(torch.from_numpy(mask.copy())), *p)
        got, stats = got.cpu().numpy(), stats.cpu().numpy()
        assert got.dtype == np.float32 and stats.dtype == np.int32, name
        assert same_bits(got, want), f"{name}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} of {want.size} pixels differ"
        assert np.array_equal(stats, wstats), f"{name}: stats {stats.tolist()} != {wstats.tolist()}"
        with np.errstate(invalid="ignore"):
            f2 = got > np.float32(p[0])
            f0 = mask > np.float32(p[0])
        assert int((f2 != f0).sum()) == int(wstats[:, 3].sum()), name


def purpose_masks(H=200, W=260):
    """(blob, raw): one solid blob; the same with three 5-pixel islands outside it and two 4-pixel pin-holes inside it."""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    blob = (((ys - H / 2) / (H * 0.3)) ** 2 + ((xs - W / 2) / (W * 0.3)) ** 2 <= 1.0).astype(np.float32)[None]
    raw = blob.copy()
    for y, x in ((12, 15), (H - 20, 30), (25, W - 30)):
        raw[0, y, x:x + 3] = 1.0
        raw[0, y + 1, x + 1] = raw[0, y - 1, x + 1] = 1.0
    for y, x in ((H // 2 - 20, W // 2 - 30), (H // 2 + 25, W // 2 + 20)):
        raw[0, y:y + 2, x:x + 2] = 0.0
    return blob, raw
