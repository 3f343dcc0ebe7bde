"""Shared by tests/test_emu_roi.py, tests/test_node_roi_cpu.py and tests/test_gpu_roi.py: the cases of the subject's box (sdm_subject_roi) with a
brute-force reference that shares no code with the kernels (csrc/k_roi.h) or with the CPU restatement (sdmatte_nodes.subject_roi), and the composition
of existing calls that sdm_apply_matte_roi must equal.  Every comparison is exact (np.array_equal / torch.equal): the box is integer arithmetic, and the
cropped call runs the same device function on the same values as the whole-frame call."""
import numpy as np
import torch

import trimap_suite as TS

ROI_KERNELS = ("roi_init", "roi_reduce", "roi_finalize")
ROI_CALL_KERNELS = ROI_KERNELS + ("roi_prep_image", "roi_prep_trimap", "roi_paste")


# ---- reference --------------------------------------------------------------------------------------------------------------------------
def brute_force(plane, roi_threshold, margin_px, margin_pct, square):
    """The definition, pixel by pixel and in Python integers: int32 [B,4] = {y0, x0, h, w}."""
    B, H, W = plane.shape
    out = np.zeros((B, 4), np.int32)
    thr = np.float32(roi_threshold)
    for b in range(B):
        pts = [(y, x) for y in range(H) for x in range(W) if plane[b, y, x] > thr] if H * W <= 4096 else None
        if pts is None:                                     # the same set through argwhere, for the sizes where the double loop takes too long
            with np.errstate(invalid="ignore"):
                pts = [tuple(p) for p in np.argwhere(plane[b] > thr)]
        if not pts:
            out[b] = (0, 0, H, W)
            continue
        ymin, ymax = min(p[0] for p in pts), max(p[0] for p in pts)
        xmin, xmax = min(p[1] for p in pts), max(p[1] for p in pts)
        bh, bw = ymax - ymin + 1, xmax - xmin + 1
        my, mx = margin_px + (bh * margin_pct) // 100, margin_px + (bw * margin_pct) // 100
        y0, y1 = max(0, ymin - my), min(H, ymax + 1 + my)
        x0, x1 = max(0, xmin - mx), min(W, xmax + 1 + mx)
        h, w = y1 - y0, x1 - x0
        if square:
            L = max(h, w)
            if h < L:
                y0 -= (L - h) // 2
                if y0 < 0:
                    y0 = 0
                if y0 + L > H:
                    y0 = max(0, H - L)
                h = min(L, H)
            elif w < L:
                x0 -= (L - w) // 2
                if x0 < 0:
                    x0 = 0
                if x0 + L > W:
                    x0 = max(0, W - L)
                w = min(L, W)
        out[b] = (y0, x0, h, w)
    return out


# ---- planes -----------------------------------------------------------------------------------------------------------------------------
def rect(H, W, y0, y1, x0, x1, B=1, value=1.0):
    p = np.zeros((B, H, W), np.float32)
    p[:, y0:y1, x0:x1] = value
    return p


def misaligned(t):
    """The same values behind a pointer that is 4 bytes off a 16-byte boundary (a slice of a larger tensor)."""
    flat = torch.empty(t.numel() + 5, dtype=t.dtype, device=t.device)
    off = 1 if flat.data_ptr() % 16 == 0 else 0
    flat = flat[off:off + t.numel()]
    flat.copy_(t.reshape(-1))
    out = flat.view(t.shape)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


SHAPES = [(1, 1), (1, 300), (257, 3), (97, 131), (300, 517)]      # 300 x 517: more than one block, W not divisible by 4


def box_cases():
    """[(name, plane fp32 [B,H,W], roi_threshold, margin_px, margin_pct, square)] - the issue's list."""
    out = []
    for H, W in SHAPES:
        tag = f"{H}x{W}"
        bl = TS.blobs(H * 1000 + W, 1, H, W, n=2)
        bl[bl < 0.45] = 0.0
        out.append((f"blobs_{tag}", bl, 0.0, 3, 10, False))
        out.append((f"blobs_square_{tag}", bl, 0.5, 2, 7, True))
    H, W = 96, 128                                                                      # W % 4 == 0: the vector path (aligned pointers)
    soft = TS.blobs(77, 1, H, W, n=3) * rect(H, W, 20, 70, 30, 110)[0]
    out.append(("vector_path_96x128", soft, 0.0, 5, 10, False))
    out.append(("soft_threshold_0.3_96x128", soft, 0.3, 5, 10, False))
    out.append(("soft_threshold_0.3_square_96x128", soft, 0.3, 5, 10, True))
    wide = TS.blobs(78, 1, 300, 516, n=4)                                               # vector path, more than one block
    wide[wide < 0.6] = 0.0
    out.append(("vector_path_blocks_300x516", wide, 0.0, 4, 5, True))
    H, W = 97, 131
    for name, (y, x) in (("top_left", (0, 0)), ("top_right", (0, W - 1)), ("bottom_left", (H - 1, 0)), ("bottom_right", (H - 1, W - 1)),
                         ("centre", (H // 2, W // 2))):
        one = np.zeros((1, H, W), np.float32)
        one[0, y, x] = 1.0
        out.append((f"single_pixel_{name}", one, 0.0, 0, 0, False))
        out.append((f"single_pixel_{name}_margin_square", one, 0.0, 6, 50, True))
    out.append(("empty", np.zeros((1, H, W), np.float32), 0.0, 4, 10, True))
    out.append(("empty_at_threshold", np.full((1, H, W), 0.3, np.float32), 0.3, 4, 10, False))      # strict >: equal is outside
    out.append(("whole_frame", np.ones((1, H, W), np.float32), 0.0, 4, 10, True))
    nan = rect(H, W, 40, 60, 50, 90)
    nan[0, ::7, ::5] = np.where(nan[0, ::7, ::5] > 0, nan[0, ::7, ::5], np.nan)          # NaN all over the background: outside U
    nan[0, 45, 60] = np.nan                                                              # ... and one inside
    out.append(("nan_is_outside", nan, 0.0, 2, 0, False))
    three = np.concatenate([rect(H, W, 10, 30, 20, 50), rect(H, W, 50, 90, 70, 120), np.zeros((1, H, W), np.float32)])
    three[2, 33, 77] = 0.7
    out.append(("batch_of_three", three, 0.0, 3, 10, False))
    out.append(("batch_of_three_square", three, 0.0, 3, 10, True))
    for name, r in (("top", (2, 20, 40, 80)), ("bottom", (80, 95, 40, 80)), ("left", (30, 60, 3, 30)), ("right", (30, 60, 100, 128))):
        out.append((f"margin_clips_{name}", rect(H, W, *r), 0.0, 20, 0, False))
    out.append(("margin_pct_not_divisible", rect(H, W, 20, 57, 30, 43), 0.0, 1, 7, False))          # 37 * 7 = 259, 13 * 7 = 91
    out.append(("margin_pct_33", rect(H, W, 20, 31, 30, 59), 0.0, 0, 33, False))                    # 11 * 33 = 363, 29 * 33 = 957
    out.append(("square_hits_top", rect(H, W, 2, 7, 30, 100), 0.0, 1, 0, True))
    out.append(("square_hits_left", rect(H, W, 10, 80, 1, 6), 0.0, 1, 0, True))
    out.append(("square_hits_bottom", rect(H, W, 90, 96, 30, 100), 0.0, 1, 0, True))
    out.append(("square_hits_right", rect(H, W, 10, 80, 125, 130), 0.0, 1, 0, True))
    out.append(("square_frame_shorter_than_L", rect(20, 200, 5, 9, 40, 140), 0.0, 2, 0, True))
    out.append(("square_frame_narrower_than_L", rect(200, 20, 40, 140, 5, 9), 0.0, 2, 0, True))
    out.append(("square_odd_growth", rect(H, W, 40, 45, 30, 60), 0.0, 0, 0, True))                  # d = 25: d / 2 rounds down
    return out


def check_subject_roi(eng, to_tensor, cases=None):
    """eng.subject_roi equals the brute force and the CPU restatement in every case, with the same three launches each; every image of a batch equals
    its own single-image call."""
    from comfyui_sdmatte_amd.sdmatte_nodes import subject_roi
    for name, plane, thr, mpx, mpct, sq in (cases if cases is not None else box_cases()):
        t = to_tensor(torch.from_numpy(plane))
        eng.lib.kernel_counts(reset=True)
        got = eng.subject_roi(t, thr, mpx, mpct, sq)
        counts = eng.lib.kernel_counts()
        assert counts == {k: 1 for k in ROI_KERNELS}, (name, counts)
        assert got.dtype == torch.int32 and tuple(got.shape) == (plane.shape[0], 4) and got.device == t.device, name
        want = brute_force(plane, thr, mpx, mpct, sq)
        assert np.array_equal(got.cpu().numpy(), want), (name, got.cpu().tolist(), want.tolist())
        assert torch.equal(got.cpu(), subject_roi(torch.from_numpy(plane), thr, mpx, mpct, sq)), name
        if plane.shape[0] > 1:
            assert len({tuple(r) for r in want.tolist()}) == plane.shape[0], name            # a different box per image
            for b in range(plane.shape[0]):
                assert torch.equal(got[b:b + 1].cpu(), eng.subject_roi(to_tensor(torch.from_numpy(plane[b:b + 1])), thr, mpx, mpct, sq).cpu()), (name, b)


# ---- sdm_apply_matte_roi == box + crop + apply_matte_node + paste + tail ----------------------------------------------------------------
H_E2E, W_E2E, S_E2E, C_E2E = 96, 128, 64, 0.8
BOX_ARGS = dict(roi_threshold=0.0, margin_px=4, margin_pct=10, square=True)


def e2e_inputs(rects, seed=5, H=H_E2E, W=W_E2E):
    """Image [B,H,W,3] and a soft plane [B,H,W] (trimap_suite.blobs) confined to one sub-rectangle (y0, y1, x0, x1) per image, 0.0 outside; the
    rectangle's own border is 0.5, so that the box of `plane > 0` is the rectangle whatever the blobs are.  Every image gets the SAME blobs."""
    B = len(rects)
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(B, H, W, 3, generator=g)
    plane = np.zeros((B, H, W), np.float32)
    for b, (y0, y1, x0, x1) in enumerate(rects):
        sub = TS.blobs(seed, 1, y1 - y0, x1 - x0, n=3)[0]
        sub[0, :] = sub[-1, :] = 0.5
        sub[:, 0] = sub[:, -1] = 0.5
        plane[b, y0:y1, x0:x1] = sub
    return image, torch.from_numpy(plane)


def reference_call(eng, to_tensor, image, trimap, mode, refine, box_args, a_crop=None):
    """(alpha, matted, roi, a_crop) from existing calls: the box on the CPU, apply_matte_node (alpha_only, no refine) on the crops - ONE call for the
    batch, so all boxes must have one size - the alpha pasted into zeros, and the node's tail on the frame."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    B, H, W = trimap.shape
    roi = N.subject_roi(trimap, **box_args)
    assert len({(int(r[2]), int(r[3])) for r in roi}) == 1, roi.tolist()
    if a_crop is None:
        ic = torch.stack([image[b, y0:y0 + h, x0:x0 + w] for b, (y0, x0, h, w) in enumerate(roi.tolist())])
        tc = torch.stack([trimap[b, y0:y0 + h, x0:x0 + w] for b, (y0, x0, h, w) in enumerate(roi.tolist())])
        a_crop, _ = eng.apply_matte_node(to_tensor(ic.contiguous()), to_tensor(tc.contiguous()), S_E2E, False, "alpha_only", False, C_E2E)
        a_crop = a_crop.cpu()
    a_full = N.paste_roi(a_crop, roi, H, W)
    alpha, matted = N.refine_and_compose(a_full, image, trimap, mode, refine, C_E2E)
    return alpha, matted, roi, a_crop


def assert_call_equals(got, want, what):
    a, m, t, r = got
    alpha, matted, roi = want
    assert r.dtype == torch.int32 and torch.equal(r.cpu(), roi), (what, r.cpu().tolist(), roi.tolist())
    assert torch.equal(a.cpu(), alpha), (what, float((a.cpu() - alpha).abs().max()))
    assert torch.equal(m.cpu(), matted), what


def count_once(eng, call):
    """Runs call() and asserts that every roi_ kernel was launched exactly once (sdm_kernel_counts)."""
    eng.lib.kernel_counts(reset=True)
    out = call()
    counts = eng.lib.kernel_counts()
    assert {k: counts.get(k) for k in ROI_CALL_KERNELS} == {k: 1 for k in ROI_CALL_KERNELS}, counts
    assert sorted(k for k in counts if k.startswith("roi_")) == sorted(ROI_CALL_KERNELS), counts
    return out


def check_roi_call_equals_composition(eng, to_tensor, modes=("alpha_only", "matted_rgba", "matted_rgb"), refines=(False, True), rects=((20, 60, 30, 90), )):
    """Every output mode with mask_refine on and off, B = len(rects) (boxes of one size at different offsets): alpha, matted and roi equal the composition;
    each roi_ kernel runs once per call (an SDM_ERR_ARENA would raise)."""
    image, trimap = e2e_inputs(rects)
    a_crop = None
    for mode in modes:
        for refine in refines:
            alpha, matted, roi, a_crop = reference_call(eng, to_tensor, image, trimap, mode, refine, BOX_ARGS, a_crop)
            assert len({tuple(r[:2]) for r in roi.tolist()}) == len(rects)                      # ... at different offsets
            got = count_once(eng, lambda: eng.apply_matte_roi(to_tensor(image), to_tensor(trimap), S_E2E, False, mode, refine, C_E2E, **BOX_ARGS))
            assert got[2] is None
            assert_call_equals(got, (alpha, matted, roi), (mode, refine))
    return image, trimap, roi


def check_roi_call_from_mask(eng, to_tensor):
    """aux_is_mask: the same with make_trimap first, and trimap_out is make_trimap's result."""
    image, mask = e2e_inputs(((25, 65, 40, 100), ), seed=6)
    thr, er, di = 0.4, 2, 3
    trimap = eng.make_trimap(to_tensor(mask), thr, er, di).cpu()
    alpha, matted, roi, _ = reference_call(eng, to_tensor, image, trimap, "matted_rgb", True, BOX_ARGS)
    got = count_once(eng, lambda: eng.apply_matte_roi(to_tensor(image), to_tensor(mask), S_E2E, False, "matted_rgb", True, C_E2E, True, thr, er, di, **BOX_ARGS))
    assert torch.equal(got[2].cpu(), trimap)
    assert_call_equals(got, (alpha, matted, roi), "from mask")


def check_roi_call_copy_shortcut(eng, to_tensor):
    """A box of exactly S x S: both preparation kernels and the way back take their copy branch, as the whole-frame kernels do on the crop."""
    image, trimap = e2e_inputs(((10, 58, 30, 78), ), seed=7)
    args = dict(roi_threshold=0.0, margin_px=8, margin_pct=0, square=False)
    alpha, matted, roi, _ = reference_call(eng, to_tensor, image, trimap, "matted_rgba", True, args)
    assert roi.tolist() == [[2, 22, S_E2E, S_E2E]]
    got = eng.apply_matte_roi(to_tensor(image), to_tensor(trimap), S_E2E, False, "matted_rgba", True, C_E2E, **args)
    assert_call_equals(got, (alpha, matted, roi), "S x S box")


def check_roi_call_empty(eng, to_tensor):
    """No pixel above the threshold: the box is the frame and the call equals apply_matte_node."""
    image, trimap = e2e_inputs(((20, 60, 30, 90), ), seed=8)
    trimap = trimap.clamp(max=0.3)
    args = dict(BOX_ARGS, roi_threshold=0.3)
    a, m, t, r = eng.apply_matte_roi(to_tensor(image), to_tensor(trimap), S_E2E, False, "matted_rgba", False, C_E2E, **args)
    a2, m2 = eng.apply_matte_node(to_tensor(image), to_tensor(trimap), S_E2E, False, "matted_rgba", False, C_E2E)
    assert r.cpu().tolist() == [[0, 0, H_E2E, W_E2E]] and t is None
    assert torch.equal(a, a2) and torch.equal(m, m2)


def check_roi_call_independent_of_outside(eng, to_tensor):
    """Other image values outside the box: the alpha stays bit-identical, matted is identical inside the box."""
    image, trimap = e2e_inputs(((20, 60, 30, 90), ), seed=9)
    a, m, _, r = eng.apply_matte_roi(to_tensor(image), to_tensor(trimap), S_E2E, False, "matted_rgba", True, C_E2E, **BOX_ARGS)
    (y0, x0, h, w), = r.cpu().tolist()
    assert 0 < h < H_E2E and 0 < w < W_E2E
    other = torch.rand(image.shape, generator=torch.Generator().manual_seed(99))
    other[:, y0:y0 + h, x0:x0 + w] = image[:, y0:y0 + h, x0:x0 + w]
    assert not torch.equal(other, image)
    a2, m2, _, r2 = eng.apply_matte_roi(to_tensor(other), to_tensor(trimap), S_E2E, False, "matted_rgba", True, C_E2E, **BOX_ARGS)
    assert torch.equal(r, r2) and torch.equal(a, a2)
    assert torch.equal(m[:, y0:y0 + h, x0:x0 + w], m2[:, y0:y0 + h, x0:x0 + w]) and not torch.equal(m, m2)
    outside = torch.ones(a.shape, dtype=torch.bool)
    outside[:, y0:y0 + h, x0:x0 + w] = False
    assert bool((a.cpu()[outside] == 0.0).all()) and float(a.max()) > 0.0                                 # outside the box: exactly 0.0


def check_roi_call_errors(eng, to_tensor):
    """An aux of another size, trimap_out without a mask and bad margins are refused, in Python and by the C ABI, with nothing written."""
    import ctypes
    import pytest
    from comfyui_sdmatte_amd.engine import _ptr
    image, trimap = e2e_inputs(((20, 60, 30, 90), ))
    image, trimap = to_tensor(image), to_tensor(trimap)
    with pytest.raises(IndexError):
        eng.apply_matte_roi(image, trimap[:, :50, :70], S_E2E, False, "alpha_only", False, C_E2E)
    with pytest.raises(ValueError):
        eng.apply_matte_roi(image, trimap[0], S_E2E, False, "alpha_only", False, C_E2E)
    with pytest.raises(ValueError):
        eng.apply_matte_roi(image, trimap, S_E2E, False, "nope", False, C_E2E)
    for bad in (dict(margin_px=-1), dict(margin_px=4097), dict(margin_px=2.5), dict(margin_pct=-1), dict(margin_pct=101), dict(roi_threshold=1.0),
                dict(roi_threshold=-0.1), dict(roi_threshold=float("nan")), dict(aux_is_mask=True, erode_px=256)):
        with pytest.raises(ValueError):
            eng.apply_matte_roi(image, trimap, S_E2E, False, "alpha_only", False, C_E2E, **bad)
    B, H, W = trimap.shape
    alpha, matted = torch.full_like(trimap, -7.0), torch.full_like(image, -7.0)
    tout, roi = torch.full_like(trimap, -7.0), torch.full((B, 4), -7, dtype=torch.int32, device=trimap.device)
    kind = eng._kind(image)

    def raw(aux_is_mask=0, thr=0.0, mpx=4, mpct=10, sq=1, tri_out=None):
        return eng.lib.sdm_apply_matte_roi(eng.h, _ptr(image), _ptr(trimap), B, H, W, S_E2E, 0, aux_is_mask, 0.5, 3, 3, thr, mpx, mpct, sq, 0, 0,
                                           ctypes.c_double(C_E2E), _ptr(alpha), _ptr(matted), _ptr(tri_out), _ptr(roi), kind, None)
    assert raw(tri_out=tout) == -1 and b"trimap_out" in eng.lib.sdm_last_error(eng.h)
    assert raw(mpx=4097) == -1 and b"margin_px" in eng.lib.sdm_last_error(eng.h)
    assert raw(mpct=101) == -1 and b"margin_pct" in eng.lib.sdm_last_error(eng.h)
    assert raw(sq=2) == -1 and b"square" in eng.lib.sdm_last_error(eng.h)
    assert raw(thr=1.0) == -1 and b"roi_threshold" in eng.lib.sdm_last_error(eng.h)
    assert raw(aux_is_mask=2) == -1
    eng.synchronize()
    for t in (alpha, matted, tout, roi):
        assert bool((t == -7).all())


def check_subject_roi_errors(eng, to_tensor):
    """Python raises ValueError; the raw C call returns SDM_ERR_INVALID (-1) with a message and leaves the output alone."""
    import pytest
    from comfyui_sdmatte_amd.engine import _ptr
    p = to_tensor(torch.rand(1, 20, 30))
    for bad in (dict(roi_threshold=1.0), dict(roi_threshold=-0.5), dict(roi_threshold=float("nan")), dict(roi_threshold=float("inf")),
                dict(roi_threshold=1.0 - 1e-9), dict(margin_px=-1), dict(margin_px=4097), dict(margin_px=1.5), dict(margin_pct=-1), dict(margin_pct=101),
                dict(margin_pct=0.5)):
        with pytest.raises(ValueError):
            eng.subject_roi(p, **bad)
    with pytest.raises(ValueError):
        eng.subject_roi(p[0])
    with pytest.raises(ValueError):
        eng.subject_roi(p[:, :0])
    with pytest.raises(ValueError):
        eng.subject_roi(p, out=torch.empty(1, 4, dtype=torch.float32, device=p.device))
    with pytest.raises(ValueError):
        eng.subject_roi(p, out=torch.empty(2, 4, dtype=torch.int32, device=p.device))
    out = torch.full((1, 4), -7, dtype=torch.int32, device=p.device)
    kind = eng._kind(p)
    for args, msg in (((1.0, 1, 1, 1), b"roi_threshold"), ((float("nan"), 1, 1, 1), b"roi_threshold"), ((-0.25, 1, 1, 1), b"roi_threshold"),
                      ((0.0, -1, 1, 1), b"outside 0 .. 4096"), ((0.0, 4097, 1, 1), b"outside 0 .. 4096"), ((0.0, 1, -1, 1), b"outside 0 .. 100"),
                      ((0.0, 1, 101, 1), b"outside 0 .. 100"), ((0.0, 1, 1, 2), b"square"), ((0.0, 1, 1, -1), b"square")):
        rc = eng.lib.sdm_subject_roi(eng.h, _ptr(p), 1, 20, 30, *args, _ptr(out), kind, None)
        assert rc == -1 and msg in eng.lib.sdm_last_error(eng.h), (args, rc, eng.lib.sdm_last_error(eng.h))
    assert eng.lib.sdm_subject_roi(eng.h, _ptr(p), 1, 0, 30, 0.0, 1, 1, 1, _ptr(out), kind, None) == -1
    assert eng.lib.sdm_subject_roi(eng.h, _ptr(p), 0, 20, 30, 0.0, 1, 1, 1, _ptr(out), kind, None) == -1
    assert eng.lib.sdm_subject_roi(eng.h, _ptr(p), 1, 20, 40000, 0.0, 1, 1, 1, _ptr(out), kind, None) == -1
    assert eng.lib.sdm_subject_roi(eng.h, _ptr(p), 1, 20, 30, 0.0, 1, 1, 1, _ptr(out), 7, None) == -1            # unknown pointer kind
    eng.synchronize()
    assert out.cpu().tolist() == [[-7, -7, -7, -7]]
    got = eng.subject_roi(p, out=out)
    assert got is out and out.cpu().tolist() != [[-7, -7, -7, -7]]
