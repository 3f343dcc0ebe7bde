"""Shared by tests/test_emu_boxes.py, tests/test_node_boxes_cpu.py and tests/test_gpu_boxes.py: the cases of a box per subject (sdm_subject_boxes) with a
brute force written from the definition in include/sdmatte.h - cleanmask_suite.components for the labelling, Python integers for the rest; it shares no
code with the kernels (csrc/k_boxes.h) or with the CPU restatement (sdmatte_nodes.subject_boxes) - and the compositions of existing calls that
sdm_apply_matte_boxes must equal.  Every comparison is exact (np.array_equal / torch.equal)."""
import numpy as np
import torch

import cleanmask_suite as CS
import roi_suite as RS
import trimap_suite as TS

VOID = [-1, 0, 0, 0, 0]
CALL_KERNELS = ("boxes_sanitize", "boxes_prep_image", "boxes_prep_trimap", "boxes_paste")


def launches(max_boxes):
    """The documented launch counts of one sdm_subject_boxes call: 8 + 2 (max_boxes - 1)."""
    out = {k: 1 for k in ("cc_tile", "cc_seam", "cc_flatten", "boxes_init", "boxes_reduce", "boxes_own", "boxes_rest", "boxes_finalize")}
    if max_boxes > 1:
        out["boxes_rank"] = 2 * (max_boxes - 1)
    return out


# ---- reference --------------------------------------------------------------------------------------------------------------------------
def box_rule(ymin, xmin, ymax, xmax, H, W, margin_px, margin_pct, square):
    """sdm_subject_roi's rule on extrema, in Python integers: [y0, x0, h, w]."""
    my, mx = margin_px + ((ymax - ymin + 1) * margin_pct) // 100, margin_px + ((xmax - xmin + 1) * margin_pct) // 100
    y0, y1, x0, x1 = max(0, ymin - my), min(H, ymax + 1 + my), max(0, xmin - mx), min(W, xmax + 1 + mx)
    h, w = y1 - y0, x1 - x0
    if square:
        L = max(h, w)
        y0 -= (L - h) // 2
        y0 = max(y0, 0)
        if y0 + L > H:
            y0 = max(0, H - L)
        x0 -= (L - w) // 2
        x0 = max(x0, 0)
        if x0 + L > W:
            x0 = max(0, W - L)
        h, w = min(L, H), min(L, W)
    return [y0, x0, h, w]


def _extrema(runs):
    return min(r[0] for r in runs), min(r[1] for r in runs), max(r[0] for r in runs), max(r[2] for r in runs) - 1


def _uncovered(run, kept):
    """The parts of the run (y, x0, x1) that lie in none of the boxes."""
    y, xa, xb = run
    segs = [(xa, xb)]
    for y0, x0, h, w in kept:
        if y0 <= y < y0 + h:
            segs = [(a, e) for s0, s1 in segs for a, e in ((s0, min(s1, x0)), (max(s0, x0 + w), s1)) if a < e]
    return [(y, a, e) for a, e in segs]


def brute_force(plane, roi_threshold, min_area, max_boxes, margin_px, margin_pct, square):
    """(boxes int32 [B,max_boxes,5], count int32 [B]) from the definition."""
    B, H, W = plane.shape
    out = np.zeros((B, max_boxes, 5), np.int32)
    out[:, :, 0] = -1
    count = np.zeros(B, np.int32)
    for b in range(B):
        with np.errstate(invalid="ignore"):
            u = plane[b] > np.float32(roi_threshold)
        comps = CS.components(u, True)                                       # ordered by root
        cands = [(sum(x1 - x0 for _, x0, x1 in c), i) for i, c in enumerate(comps)]
        cands = sorted((c for c in cands if c[0] >= min_area), key=lambda c: (-c[0], c[1]))[:max_boxes - 1]
        kept = []
        for _, i in cands:
            ymin, xmin, ymax, xmax = _extrema(comps[i])
            if any(y0 <= ymin and ymax < y0 + h and x0 <= xmin and xmax < x0 + w for y0, x0, h, w in kept):
                continue
            kept.append(box_rule(ymin, xmin, ymax, xmax, H, W, margin_px, margin_pct, square))
        rest = [(y, a, e) for c in comps for run in c for y, a, e in _uncovered(run, kept)]      # runs of R
        entries = list(kept)
        if rest:
            entries.append(box_rule(*_extrema(rest), H, W, margin_px, margin_pct, square))
        if not entries:
            assert not comps
            entries.append([0, 0, H, W])
        for i, e in enumerate(entries):
            out[b, i] = [b] + e
        count[b] = len(entries)
    return out, count


def covered(plane, roi_threshold, boxes):
    """The coverage invariant, by brute force: every pixel of U lies in at least one box of its image."""
    B, H, W = plane.shape
    for b in range(B):
        cover = np.zeros((H, W), bool)
        for bb, y0, x0, h, w in boxes[b].tolist():
            if bb >= 0:
                assert bb == b and 0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= H and x0 + w <= W, (b, bb, y0, x0, h, w)
                cover[y0:y0 + h, x0:x0 + w] = True
        with np.errstate(invalid="ignore"):
            if bool(((plane[b] > np.float32(roi_threshold)) & ~cover).any()):
                return False
    return True


# ---- planes -----------------------------------------------------------------------------------------------------------------------------
def paint(H, W, rects, B=1):
    p = np.zeros((B, H, W), np.float32)
    for y0, y1, x0, x1 in rects:
        p[:, y0:y1, x0:x1] = 1.0
    return p


THREE = ((10, 40, 10, 50), (50, 70, 70, 100), (80, 90, 20, 32))             # areas 1200, 600, 120 in 97 x 131


def box_cases(big=False):
    """[(name, plane fp32 [B,H,W], roi_threshold, min_area, max_boxes, margin_px, margin_pct, square)] - the issue's list."""
    out = []
    for H, W in RS.SHAPES:
        bl = TS.blobs(H * 1000 + W, 1, H, W, n=3)
        bl[bl < 0.45] = 0.0
        out.append((f"blobs_{H}x{W}", bl, 0.0, 4, 4, 3, 10, False))
        out.append((f"blobs_square_{H}x{W}", bl, 0.5, 1, 3, 2, 7, True))
    soft = TS.blobs(77, 1, 96, 128, n=3) * (paint(96, 128, ((8, 40, 10, 60), (50, 90, 70, 120)))[0])
    out.append(("vector_path_96x128", soft, 0.0, 16, 4, 5, 10, False))
    out.append(("vector_path_96x128_soft_square", soft, 0.3, 16, 3, 5, 10, True))
    H, W = 97, 131
    for K in (1, 2, 3, 4, 8):
        out.append((f"three_blobs_K{K}", paint(H, W, THREE), 0.0, 64, K, 2, 5, False))
    out.append(("area_tie_smaller_root_wins", paint(H, W, ((60, 70, 80, 100), (10, 30, 10, 20), (40, 45, 40, 45))), 0.0, 1, 2, 1, 0, False))
    for name, ma in (("at", 120), ("below", 119), ("above", 121)):
        # (the speck keeps the cases apart: below min_area the third blob shares the rest box with it)
        out.append((f"min_area_{name}_the_area", paint(H, W, THREE + ((2, 4, 120, 123), )), 0.0, ma, 8, 0, 0, False))
    # a 3 x 3 hand 5 pixels right of the large blob: inside its margin box of 6 (columns up to 55), one pixel outside it when it starts at column 56
    out.append(("small_inside_margin_box_dropped", paint(H, W, ((10, 40, 10, 50), (20, 23, 53, 56))), 0.0, 4, 4, 6, 0, False))
    out.append(("small_one_pixel_outside_kept", paint(H, W, ((10, 40, 10, 50), (20, 23, 54, 57))), 0.0, 4, 4, 6, 0, False))
    out.append(("small_one_pixel_outside_to_rest", paint(H, W, ((10, 40, 10, 50), (20, 23, 54, 57))), 0.0, 10, 4, 6, 0, False))
    sp = paint(H, W, ((10, 40, 10, 50), (50, 70, 70, 100)))
    g = np.random.default_rng(5)
    sp[0].ravel()[g.choice(H * W, 200, replace=False)] = 1.0
    out.append(("speckle_gives_the_rest_box", sp, 0.0, 64, 4, 2, 5, False))
    many = paint(H, W, [(5 + 18 * i, 5 + 18 * i + 6 + i, 8 + 20 * j, 8 + 20 * j + 9) for i in range(5) for j in range(6)])
    out.append(("more_candidates_than_slots", many, 0.0, 4, 4, 1, 0, False))
    out.append(("more_candidates_than_slots_K8_square", many, 0.0, 4, 8, 1, 10, True))
    out.append(("empty", np.zeros((1, H, W), np.float32), 0.0, 4, 4, 4, 10, True))
    out.append(("empty_at_threshold", np.full((1, H, W), 0.3, np.float32), 0.3, 4, 4, 4, 10, False))
    out.append(("whole_frame", np.ones((1, H, W), np.float32), 0.0, 4, 4, 4, 10, True))
    nan = paint(H, W, ((40, 60, 50, 90), (5, 15, 5, 25)))
    nan[0, ::7, ::5] = np.where(nan[0, ::7, ::5] > 0, nan[0, ::7, ::5], np.nan)
    nan[0, 45, 60] = np.nan
    out.append(("nan_is_outside", nan, 0.0, 4, 4, 2, 0, False))
    diag = np.zeros((1, H, W), np.float32)
    diag[0, np.arange(10, 70), np.arange(100, 40, -1)] = 1.0                # an anti-diagonal: NE links only
    diag[0, np.arange(5, 40), np.arange(5, 40)] = 1.0
    out.append(("diagonal_lines_are_connected", diag, 0.0, 20, 4, 0, 0, False))
    edges = paint(H, W, ((0, 12, 40, 70), (H - 9, H, 20, 60), (30, 60, 0, 7), (25, 70, W - 11, W)))
    out.append(("edges_margins_clip", edges, 0.0, 4, 8, 20, 0, False))
    out.append(("edges_square_shifts", edges, 0.0, 4, 8, 1, 10, True))
    three = np.concatenate([paint(H, W, THREE), paint(H, W, ((50, 90, 70, 120), (3, 8, 3, 9))), np.zeros((1, H, W), np.float32)])
    three[2, 33, 77] = 0.7
    out.append(("batch_of_three", three, 0.0, 16, 4, 3, 10, False))
    out.append(("batch_of_three_square", three, 0.0, 16, 3, 3, 10, True))
    if big:
        pl = TS.blobs(41, 2, 1080, 1920, n=4)
        pl[pl < 0.5] = 0.0
        pl[1, 1079, 1919] = 0.25
        pl[0, 3, 1900:1903] = 0.25
        out.append(("many_blocks_1080x1920", pl, 0.0, 64, 4, 16, 10, True))
    return out


def check_subject_boxes(eng, to_tensor, cases=None):
    """eng.subject_boxes equals the brute force and the CPU restatement in every case, with the documented launches; coverage; void entries; every image of
    a batch equals its own single-image call; max_boxes = 1 equals subject_roi."""
    from comfyui_sdmatte_amd.sdmatte_nodes import subject_boxes
    for name, plane, thr, ma, K, mpx, mpct, sq in (cases if cases is not None else box_cases()):
        t = to_tensor(torch.from_numpy(plane))
        B = plane.shape[0]
        eng.lib.kernel_counts(reset=True)
        got, cnt = eng.subject_boxes(t, thr, ma, K, mpx, mpct, sq, return_count=True)
        counts = eng.lib.kernel_counts()
        assert counts == launches(K), (name, counts)
        assert got.dtype == torch.int32 and tuple(got.shape) == (B, K, 5) and got.device == t.device and cnt.dtype == torch.int32 and tuple(cnt.shape) == (B, ), name
        want, wcnt = brute_force(plane, thr, ma, K, mpx, mpct, sq)
        g, c = got.cpu().numpy(), cnt.cpu().numpy()
        assert np.array_equal(g, want) and np.array_equal(c, wcnt), (name, g.tolist(), want.tolist(), c.tolist(), wcnt.tolist())
        rb, rc = subject_boxes(torch.from_numpy(plane), thr, ma, K, mpx, mpct, sq, return_count=True)
        assert np.array_equal(g, rb.numpy()) and np.array_equal(c, rc.numpy()), name
        assert covered(plane, thr, g), name
        for b in range(B):
            assert 1 <= c[b] <= K and all(e == VOID for e in g[b, c[b]:].tolist()) and all(e[0] == b for e in g[b, :c[b]].tolist()), (name, g.tolist())
        one = eng.subject_boxes(t, thr, ma, 1, mpx, mpct, sq)
        roi = eng.subject_roi(t, thr, mpx, mpct, sq)
        assert torch.equal(one[:, 0, 1:], roi) and one[:, 0, 0].tolist() == list(range(B)), name
        if B > 1:
            for b in range(B):
                single = eng.subject_boxes(to_tensor(torch.from_numpy(plane[b:b + 1])), thr, ma, K, mpx, mpct, sq).cpu()
                assert torch.equal(got[b, :, 1:].cpu(), single[0, :, 1:]), (name, b)


def check_subject_boxes_errors(eng, to_tensor):
    """Python raises ValueError; the raw C call returns SDM_ERR_INVALID (-1) with a message and leaves the outputs alone."""
    import pytest
    from comfyui_sdmatte_amd.engine import _ptr
    p = to_tensor(torch.rand(1, 20, 30))
    for bad in (dict(roi_threshold=1.0), dict(roi_threshold=float("nan")), dict(margin_px=-1), dict(margin_px=4097), dict(margin_pct=101), dict(min_area=-1),
                dict(min_area=(1 << 28) + 1), dict(min_area=1.5), dict(max_boxes=0), dict(max_boxes=9), dict(max_boxes=2.5)):
        with pytest.raises(ValueError):
            eng.subject_boxes(p, **bad)
    with pytest.raises(ValueError):
        eng.subject_boxes(p[0])
    with pytest.raises(ValueError):
        eng.subject_boxes(p, out=torch.empty(1, 4, 4, dtype=torch.int32, device=p.device))
    out = torch.full((1, 4, 5), -7, dtype=torch.int32, device=p.device)
    cnt = torch.full((1, ), -7, dtype=torch.int32, device=p.device)
    kind = eng._kind(p)
    for args, msg in (((1.0, 4, 4, 1, 1, 1), b"roi_threshold"), ((0.0, -1, 4, 1, 1, 1), b"min_area"), ((0.0, (1 << 28) + 1, 4, 1, 1, 1), b"min_area"),
                      ((0.0, 4, 0, 1, 1, 1), b"max_boxes"), ((0.0, 4, 9, 1, 1, 1), b"max_boxes"), ((0.0, 4, 4, 4097, 1, 1), b"margin_px"),
                      ((0.0, 4, 4, 1, 101, 1), b"margin_pct"), ((0.0, 4, 4, 1, 1, 2), b"square")):
        rc = eng.lib.sdm_subject_boxes(eng.h, _ptr(p), 1, 20, 30, *args, _ptr(out), _ptr(cnt), kind, None)
        assert rc == -1 and msg in eng.lib.sdm_last_error(eng.h), (args, rc, eng.lib.sdm_last_error(eng.h))
    assert eng.lib.sdm_subject_boxes(eng.h, _ptr(p), 1, 0, 30, 0.0, 4, 4, 1, 1, 1, _ptr(out), _ptr(cnt), kind, None) == -1
    assert eng.lib.sdm_subject_boxes(eng.h, _ptr(p), 1, 20, 40000, 0.0, 4, 4, 1, 1, 1, _ptr(out), _ptr(cnt), kind, None) == -1
    assert eng.lib.sdm_subject_boxes(eng.h, _ptr(p), 1, 20, 30, 0.0, 4, 4, 1, 1, 1, _ptr(out), _ptr(cnt), 7, None) == -1
    eng.synchronize()
    assert bool((out == -7).all()) and bool((cnt == -7).all())
    got = eng.subject_boxes(p, out=out)
    assert got is out and not bool((out == -7).any())


# ---- sdm_apply_matte_boxes ----------------------------------------------------------------------------------------------------------------
H_E2E, W_E2E, S_E2E, C_E2E = RS.H_E2E, RS.W_E2E, RS.S_E2E, RS.C_E2E


def frames(B, seed=21, H=H_E2E, W=W_E2E):
    """Image [B,H,W,3] and a soft trimap [B,H,W] that differs from pixel to pixel and image to image."""
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(B, H, W, 3, generator=g)
    trimap = torch.from_numpy(np.concatenate([TS.blobs(seed + b, 1, H, W, n=4) for b in range(B)]))
    return image, trimap


def boxes_tensor(entries):
    return torch.tensor(entries, dtype=torch.int32).reshape(-1, 5)


def composition(eng, to_tensor, image, trimap, boxes, mode, refine):
    """(alpha, matted, crops) from existing calls: crops by hand, ONE apply_matte_node call of batch N on them (alpha_only, no refine; so all boxes have
    one size), the crops pasted into zeros with an element-wise maximum per image (sdmatte_nodes.paste_boxes), the node's tail on the frame."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    B, H, W = trimap.shape
    ic = torch.stack([image[b, y0:y0 + h, x0:x0 + w] for b, y0, x0, h, w in boxes.tolist()]).contiguous()
    tc = torch.stack([trimap[b, y0:y0 + h, x0:x0 + w] for b, y0, x0, h, w in boxes.tolist()]).contiguous()
    crops, _ = eng.apply_matte_node(to_tensor(ic), to_tensor(tc), S_E2E, False, "alpha_only", False, C_E2E)
    crops = crops.cpu()
    alpha, matted = N.refine_and_compose(N.paste_boxes(crops, boxes, B, H, W), image, trimap, mode, refine, C_E2E)
    return alpha, matted, crops


def call(eng, to_tensor, image, trimap, boxes, mode="alpha_only", refine=False, **kw):
    return eng.apply_matte_boxes(to_tensor(image), to_tensor(trimap), to_tensor(boxes), S_E2E, False, mode, refine, C_E2E, **kw)


def count_once(eng, fn):
    """Runs fn() and asserts that every boxes_ kernel of the call was launched exactly once (sdm_kernel_counts)."""
    eng.lib.kernel_counts(reset=True)
    out = fn()
    counts = eng.lib.kernel_counts()
    assert {k: v for k, v in counts.items() if k.startswith("boxes_")} == {k: 1 for k in CALL_KERNELS}, counts
    assert not any(k.startswith("roi_") for k in counts), counts
    return out


def check_equals_roi_call(eng, to_tensor):
    """Equality 1: the list {b, roi[b]} of subject_roi, two images with boxes of different sizes, against apply_matte_roi, in alpha and matted."""
    image, trimap = RS.e2e_inputs(((20, 60, 30, 90), (5, 80, 60, 120)), seed=11)
    args = dict(roi_threshold=0.0, margin_px=3, margin_pct=5, square=False)
    for mode, refine in (("matted_rgba", True), ("alpha_only", False)):
        a, m, _, roi = eng.apply_matte_roi(to_tensor(image), to_tensor(trimap), S_E2E, False, mode, refine, C_E2E, **args)
        assert roi[0, 2:].tolist() != roi[1, 2:].tolist()
        boxes = torch.cat([torch.arange(2, dtype=torch.int32).reshape(2, 1), roi.cpu()], 1)
        a2, m2 = count_once(eng, lambda: call(eng, to_tensor, image, trimap, boxes, mode, refine))
        assert torch.equal(a, a2) and torch.equal(m, m2), (mode, refine, float((a - a2).abs().max()))


def check_equals_composition(eng, to_tensor, entries, B=1, modes=(("alpha_only", False), ), overlap=None, seed=21):
    """Equality 2: boxes of one common size against the composition of existing calls.  overlap = (y0, y1, x0, x1): a frame region that lies in boxes 0 and
    1, where the two crops must really differ, so that the maximum is exercised."""
    image, trimap = frames(B, seed)
    boxes = boxes_tensor(entries)
    crops = None
    for mode, refine in modes:
        alpha, matted, crops = composition(eng, to_tensor, image, trimap, boxes, mode, refine)
        a, m = count_once(eng, lambda: call(eng, to_tensor, image, trimap, boxes, mode, refine))
        assert torch.equal(a.cpu(), alpha), (entries, mode, refine, float((a.cpu() - alpha).abs().max()))
        assert torch.equal(m.cpu(), matted), (entries, mode, refine)
    if overlap is not None:
        y0, y1, x0, x1 = overlap
        (_, ya, xa, _, _), (_, yb, xb, _, _) = entries[0], entries[1]
        ca, cb = crops[0][y0 - ya:y1 - ya, x0 - xa:x1 - xa], crops[1][y0 - yb:y1 - yb, x0 - xb:x1 - xb]
        assert ca.shape == cb.shape == (y1 - y0, x1 - x0) and bool((ca > cb).any()) and bool((cb > ca).any())
    return image, trimap, boxes


BAD_ENTRIES = ([-1, 0, 0, 0, 0], [2, 5, 5, 40, 40], [-3, 5, 5, 40, 40], [0, 5, 5, 0, 40], [0, 5, 5, 40, 0], [0, -1, 5, 40, 40], [0, 5, -1, 40, 40],
               [0, 60, 5, 40, 40], [0, 5, 100, 40, 40], [0, 2147483647, 5, 2147483647, 40], [0, 5, 2147483600, 40, 2147483600])


def check_void_entries(eng, to_tensor):
    """A void entry in the middle and one entry per violated clause of the validity rule (two of them overflow 32-bit sums), B = 2 with both valid boxes in
    image 1.  A void slot is fed the whole frame of image 0, so the list with every bad entry replaced by {0, 0, 0, H, W} runs the same model batch: on
    the images of the compacted list (image 1) the two calls are equal bit for bit.  (The call on the compacted list itself has another N, and the model's
    kernels are chosen by launch size: its bits may differ.)  Image 0, which has no valid box, gets alpha exactly 0.0, as does everything outside the
    valid boxes."""
    from comfyui_sdmatte_amd.sdmatte_nodes import compact_boxes
    image, trimap = frames(2, seed=23)
    good = [[1, 10, 20, 48, 48], [1, 40, 70, 48, 48]]
    entries = [good[0]] + [list(e) for e in BAD_ENTRIES] + [good[1]]
    boxes = boxes_tensor(entries)
    assert len(entries) == 13 and compact_boxes(boxes).shape[0] == 11           # compact_boxes only knows the void mark: the other bad ones stay for the device
    same_batch = boxes_tensor([good[0]] + [[0, 0, 0, H_E2E, W_E2E]] * len(BAD_ENTRIES) + [good[1]])
    # the raw call into the middle of buffers filled with -7: nothing is written outside the outputs
    import ctypes
    from comfyui_sdmatte_amd.engine import _ptr
    img, tri, lst = to_tensor(image), to_tensor(trimap), to_tensor(boxes)
    px, guard = trimap.numel(), 4096
    abuf, mbuf = torch.full((px + 2 * guard, ), -7.0, device=img.device), torch.full((px * 4 + 2 * guard, ), -7.0, device=img.device)
    rc = eng.lib.sdm_apply_matte_boxes(eng.h, _ptr(img), _ptr(tri), 2, H_E2E, W_E2E, S_E2E, 0, _ptr(lst), lst.shape[0], 1, 1, ctypes.c_double(C_E2E),
                                       _ptr(abuf[guard:]), _ptr(mbuf[guard:]), eng._kind(img), None)
    eng.synchronize()
    assert rc == 0
    for buf, n in ((abuf, px), (mbuf, 4 * px)):
        assert bool((buf[:guard] == -7).all()) and bool((buf[guard + n:] == -7).all())
    a, m = abuf[guard:guard + px].view(2, H_E2E, W_E2E), mbuf[guard:guard + 4 * px].view(2, H_E2E, W_E2E, 4)
    a2, m2 = call(eng, to_tensor, image, trimap, same_batch, "matted_rgba", True)
    assert torch.equal(a[1], a2[1]) and torch.equal(m[1], m2[1])
    assert bool((a[0] == 0.0).all()) and float(a[1].max()) > 0.0 and float(a2[0].max()) > 0.0
    outside = torch.ones(a[1].shape, dtype=torch.bool)
    for _, y0, x0, h, w in good:
        outside[y0:y0 + h, x0:x0 + w] = False
    assert bool((a[1].cpu()[outside] == 0.0).all())
    a0, _ = call(eng, to_tensor, image, trimap, boxes_tensor([VOID]))                             # no valid entry at all
    assert bool((a0 == 0.0).all())


def check_call_errors(eng, to_tensor):
    """N = 0, N = 17 and a bad output_mode are SDM_ERR_INVALID with a message at the C ABI (a trimap of another size cannot be said there: the planes share
    B, H, W; Python refuses it with IndexError); outputs pre-filled with -7 stay untouched."""
    import ctypes
    import pytest
    from comfyui_sdmatte_amd.engine import _ptr
    image, trimap = frames(1)
    image, trimap = to_tensor(image), to_tensor(trimap)
    ok = to_tensor(boxes_tensor([[0, 10, 20, 48, 48]]))
    with pytest.raises(IndexError):
        eng.apply_matte_boxes(image, trimap[:, :50, :70], ok, S_E2E, False, "alpha_only", False, C_E2E)
    for bad in ((image, trimap[0], ok, "alpha_only"), (image, trimap, ok, "nope"), (image, trimap, ok[:0], "alpha_only"), (image, trimap, ok.repeat(17, 1), "alpha_only"),
                (image, trimap, ok.float(), "alpha_only"), (image, trimap, ok[:, :4], "alpha_only"), (image[..., :2], trimap, ok, "alpha_only")):
        with pytest.raises(ValueError):
            eng.apply_matte_boxes(bad[0], bad[1], bad[2], S_E2E, False, bad[3], False, C_E2E)
    B, H, W = trimap.shape
    alpha, matted = torch.full_like(trimap, -7.0), torch.full_like(image, -7.0)
    lst = to_tensor(boxes_tensor([[0, 10, 20, 48, 48]] * 17))
    kind = eng._kind(image)

    def raw(N=1, mode=0, S=S_E2E, H_=H):
        return eng.lib.sdm_apply_matte_boxes(eng.h, _ptr(image), _ptr(trimap), B, H_, W, S, 0, _ptr(lst), N, mode, 0, ctypes.c_double(C_E2E), _ptr(alpha),
                                             _ptr(matted), kind, None)
    assert raw(N=0) == -1 and b"N = 0" in eng.lib.sdm_last_error(eng.h)
    assert raw(N=17) == -1 and b"N = 17" in eng.lib.sdm_last_error(eng.h)
    assert raw(mode=3) == -1 and b"output mode" in eng.lib.sdm_last_error(eng.h)
    assert raw(mode=-1) == -1
    assert raw(S=65) == -1 and b"multiple of 64" in eng.lib.sdm_last_error(eng.h)
    assert raw(H_=0) == -1 and b"bad plane size" in eng.lib.sdm_last_error(eng.h)
    eng.synchronize()
    assert bool((alpha == -7).all()) and bool((matted == -7).all())
