"""Shared by tests/test_emu_canvas.py, tests/test_node_canvas_cpu.py and tests/test_gpu_canvas.py: the cases of the cut-out on a canvas (sdm_compose_canvas,
csrc/k_canvas.h) and their checks.  Placements are compared exactly with sdmatte_nodes.canvas_fit(subject_roi(...)); values with
sdmatte_nodes.compose_canvas(dtype=float64).

Tolerance.  MEASURED_F32_DEVIATION is the largest deviation of compose_canvas(dtype=float32) from compose_canvas(dtype=float64) over every case below, on the
CPU, in the quantities that are compared (A and the premultiplied A*rgb everywhere, straight rgb where A >= 1/64): 2.8e-6 (2.788e-6 measured), reached by a straight colour at a
small alpha (the division by A amplifies the rounding of P up to 64 times).  The bound is four times that, TOL = 1.12e-5: the
kernel sums in another order than torch, and the torchvision-style weights are normalised in fp32.  test_node_canvas_cpu.py repeats the measurement
and checks that the pixels left out of the straight comparison (0 < A < 1/64) are at most 5 % of the pixels with A > 0."""
import numpy as np
import torch

MEASURED_F32_DEVIATION = 2.8e-6
TOL = 4 * MEASURED_F32_DEVIATION
A_MIN = 1.0 / 64.0

BOX_KERNELS = ("roi_init", "roi_reduce", "roi_finalize", "canvas_fit")
PLAIN_KERNELS = BOX_KERNELS + ("canvas_compose", )
SHADOW_KERNELS = BOX_KERNELS + ("canvas_place", "canvas_blur_rows", "canvas_blur_compose")


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def disc(H, W, cy, cx, ry, rx, ramp=3.0):
    """A soft ellipse: 1 inside, 0 outside, a linear ramp of about `ramp` pixels between."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.sqrt(((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2)
    return np.clip((1.0 - d) * min(ry, rx) / ramp + 0.5, 0.0, 1.0).astype(np.float32)


def colours(seed, B, H, W):
    return torch.rand(B, H, W, 3, generator=torch.Generator().manual_seed(seed))


def _case(name, fg, alpha, canvas_h, canvas_w, **kw):
    alpha = torch.from_numpy(np.ascontiguousarray(alpha)) if isinstance(alpha, np.ndarray) else alpha
    return (name, fg, alpha, dict(canvas_h=canvas_h, canvas_w=canvas_w, **kw))


def cases():
    """[(name, fg [B,H,W,3], alpha [B,H,W], keyword arguments of compose_canvas)]"""
    out = []
    H, W = 37, 53
    two = np.stack([disc(H, W, 18, 26, 17, 25), disc(H, W, 20, 27, 14, 24)])                 # boxes of about 35 x 51 and 29 x 49
    fg2 = colours(1, 2, H, W)
    grey = (0.5, 0.25, 0.75)
    out.append(_case("downscale_b2_rgba", fg2, two, 32, 48, fill_pct=80))
    out.append(_case("downscale_b2_colour_rgb", fg2, two, 32, 48, fill_pct=80, bg_color=grey))
    out.append(_case("downscale_b2_colour_rgba", fg2, two, 32, 48, fill_pct=80, bg_color=grey, out_channels=4))
    bg1, bgB = colours(2, 1, 32, 48), colours(3, 2, 32, 48)
    out.append(_case("downscale_b2_image_batch1", fg2, two, 32, 48, fill_pct=80, bg_image=bg1))
    out.append(_case("downscale_b2_image_batchB_rgba", fg2, two, 32, 48, fill_pct=80, bg_image=bgB, out_channels=4))
    out.append(_case("odd_canvas_rgb_runs", fg2, two, 31, 45, fill_pct=90, bg_color=grey))                     # 45 % 4 != 0: runs of 4 cross rows and images
    up = disc(24, 20, 11, 10, 8, 6)[None]
    out.append(_case("upscale_fill100", colours(4, 1, 24, 20), up, 64, 40, fill_pct=100))
    # a box of 20 x 16 whose fitted size is 20 x 16: th = 25 * 80 / 100 = 20, dw = (16 * 20 + 10) / 20 = 16
    cp = np.zeros((1, 40, 40), np.float32)
    cp[0, 5:25, 8:24] = np.random.default_rng(5).uniform(0.2, 1.0, (20, 16)).astype(np.float32) * disc(20, 16, 9.5, 7.5, 12, 10)
    cp[0, 5, 8] = cp[0, 24, 23] = 0.6
    out.append(_case("copy_branch", colours(5, 1, 40, 40), cp, 25, 40, fill_pct=80, valign="top"))
    out.append(_case("copy_branch_shadow_colour", colours(5, 1, 40, 40), cp, 25, 40, fill_pct=80, bg_color=grey, shadow_opacity=0.6, shadow_sigma=1.0, shadow_dy=2,
                     shadow_dx=1))
    out.append(_case("empty_alpha", colours(6, 1, 24, 20), np.zeros((1, 24, 20), np.float32), 32, 48, fill_pct=80))
    out.append(_case("empty_alpha_colour", colours(6, 1, 24, 20), np.zeros((1, 24, 20), np.float32), 32, 48, fill_pct=80, bg_color=grey))
    nan = disc(H, W, 18, 26, 12, 16)[None].copy()
    nan[0, ::5, ::7] = np.nan
    nan[0, 2, 3] = np.inf
    out.append(_case("nan_alpha", colours(7, 1, H, W), nan, 32, 48, fill_pct=80, bg_color=grey, out_channels=4))
    out.append(_case("edge_box", colours(8, 1, H, W), disc(H, W, 3, 48, 10, 12)[None], 32, 48, fill_pct=80))
    tall, wide = disc(H, W, 18, 26, 16, 6)[None], disc(H, W, 18, 26, 5, 22)[None]
    for fill in (100, 50, 1):
        for valign in (0, 1, 2):
            src, nm = (tall, "tall") if (fill + valign) % 2 == 0 else (wide, "wide")
            out.append(_case(f"fit_{nm}_fill{fill}_valign{valign}", colours(9, 1, H, W), src, 32, 48, fill_pct=fill, valign=valign))
    out.append(_case("fit_tall_square_canvas", colours(9, 1, H, W), tall, 40, 40, fill_pct=70, valign="bottom", bg_color=grey))
    out.append(_case("fit_wide_square_canvas", colours(9, 1, H, W), wide, 40, 40, fill_pct=70, valign="bottom", bg_color=grey))
    out.append(_case("threshold_0.5", fg2, two, 32, 48, fill_pct=80, roi_threshold=0.5))
    # shadows
    out.append(_case("shadow_leaves_canvas_colour", fg2, two, 32, 48, fill_pct=90, bg_color=grey, shadow_opacity=0.7, shadow_sigma=1.5, shadow_dy=3, shadow_dx=-2))
    out.append(_case("shadow_transparent", fg2, two, 32, 48, fill_pct=70, shadow_opacity=0.7, shadow_sigma=1.5, shadow_dy=3, shadow_dx=-2))
    out.append(_case("shadow_image_rgb_odd_canvas", fg2, two, 31, 45, fill_pct=70, bg_image=colours(10, 2, 31, 45), shadow_opacity=1.0, shadow_sigma=2.0, shadow_dy=-4,
                     shadow_dx=5))
    out.append(_case("shadow_sigma32_canvas40", colours(4, 1, 24, 20), up, 40, 40, fill_pct=60, bg_color=grey, shadow_opacity=0.9, shadow_sigma=32.0, shadow_dy=1,
                     shadow_dx=1))
    out.append(_case("shadow_two_tiles", colours(4, 1, 24, 20), up, 70, 130, fill_pct=80, valign="bottom", bg_color=grey, out_channels=4, shadow_opacity=0.5, shadow_sigma=3.0,
                     shadow_dy=40, shadow_dx=-70))
    return out


# ---- comparison -------------------------------------------------------------------------------------------------------------------------
def deviation(got, want):
    """(largest deviation in the compared quantities, pixels with A > 0, pixels with 0 < A < 1/64) of a result [B,h,w,3|4] against the float64 one."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.shape[-1] == 3:
        return float((got - want).abs().max()), 0, 0
    Ag, Aw = got[..., 3:], want[..., 3:]
    d = max(float((Ag - Aw).abs().max()), float((Ag * got[..., :3] - Aw * want[..., :3]).abs().max()))
    solid = (Aw >= A_MIN).expand_as(want[..., :3])
    if bool(solid.any()):
        d = max(d, float((got[..., :3] - want[..., :3])[solid].abs().max()))
    return d, int((Aw > 0).sum()), int(((Aw > 0) & (Aw < A_MIN)).sum())


def reference(fg, alpha, kw, dtype=torch.float64):
    from comfyui_sdmatte_amd.sdmatte_nodes import compose_canvas
    return compose_canvas(fg, alpha, dtype=dtype, return_placement=True, **kw)


_REF = {}


def reference64(case):
    """The float64 evaluation of a case, computed once and shared."""
    name, fg, alpha, kw = case
    if name not in _REF:
        _REF[name] = reference(fg, alpha, kw)
    return _REF[name]


def _dev_kw(kw, to_tensor):
    return {k: (to_tensor(v) if k == "bg_image" else v) for k, v in kw.items()}


def check_case(eng, to_tensor, case):
    """One engine call: the placement equals canvas_fit(subject_roi(...)) exactly and lies inside the canvas, the launches are those of the header, the values
    are within TOL of the float64 restatement."""
    from comfyui_sdmatte_amd.sdmatte_nodes import canvas_fit, subject_roi
    name, fg, alpha, kw = case
    want, wplace = reference64(case)
    eng.lib.kernel_counts(reset=True)
    got, place = eng.compose_canvas(to_tensor(fg), to_tensor(alpha), return_placement=True, **_dev_kw(kw, to_tensor))
    counts = eng.lib.kernel_counts()
    assert counts == {k: 1 for k in (SHADOW_KERNELS if kw.get("shadow_opacity", 0.0) > 0 else PLAIN_KERNELS)}, (name, counts)
    assert place.dtype == torch.int32 and tuple(place.shape) == (fg.shape[0], 8), name
    fit = canvas_fit(subject_roi(alpha, kw.get("roi_threshold", 0.0), 0, 0, False), kw["canvas_h"], kw["canvas_w"], kw.get("fill_pct", 80), kw.get("valign", "center"))
    assert torch.equal(place.cpu(), fit) and torch.equal(wplace, fit), (name, place.cpu().tolist(), fit.tolist())
    y0, x0, h, w, dy0, dx0, dh, dw = (fit[:, k] for k in range(8))
    assert bool(((dy0 >= 0) & (dx0 >= 0) & (dh >= 1) & (dw >= 1) & (dy0 + dh <= kw["canvas_h"]) & (dx0 + dw <= kw["canvas_w"])).all()), (name, fit.tolist())
    assert got.dtype == torch.float32 and got.shape == want.shape and got.device == to_tensor(fg).device, name
    assert bool(torch.isfinite(got).all()), name
    d, _, _ = deviation(got, want)
    print(f"canvas {name}: deviation {d:.3e} (bound {TOL:.3e})")
    assert d <= TOL, (name, d, TOL)
    if kw.get("bg_color") is not None or kw.get("bg_image") is not None:
        if got.shape[-1] == 4:
            assert bool((got[..., 3] == 1.0).all()), name                      # an opaque background: A == 1.0 exactly
    return got, place


def check_all(eng, to_tensor, select=None):
    names = []
    for case in cases():
        if select is None or select(case[0]):
            check_case(eng, to_tensor, case)
            names.append(case[0])
    return names


# ---- premultiplication ------------------------------------------------------------------------------------------------------------------
GREY = 0.5


def premult_scene():
    """Pure red where alpha = 0, grey elsewhere; the box of the disc is 32 x 32 and lands at 16 x 16 (a reduction by 2) on a grey canvas."""
    a = disc(40, 40, 19.5, 19.5, 16, 16, ramp=2.0)
    a[:4] = a[36:] = 0.0
    a[:, :4] = a[:, 36:] = 0.0
    fg = torch.full((1, 40, 40, 3), GREY)
    red = torch.from_numpy(a == 0)
    fg[0][red] = torch.tensor([1.0, 0.0, 0.0])
    kw = dict(canvas_h=20, canvas_w=20, fill_pct=80, bg_color=(GREY, GREY, GREY))
    return fg, torch.from_numpy(a)[None], kw


def straight_resample(fg, alpha, place, kw):
    """What a generic resize node does: the STRAIGHT colours and the alpha resized on their own, then composed over the grey."""
    import torch.nn.functional as F
    (y0, x0, h, w, dy0, dx0, dh, dw), = place.tolist()
    c = F.interpolate(fg[:, y0:y0 + h, x0:x0 + w].permute(0, 3, 1, 2), size=(dh, dw), mode="bilinear", antialias=True)
    a = F.interpolate(alpha[:, None, y0:y0 + h, x0:x0 + w], size=(dh, dw), mode="bilinear", antialias=True)
    out = torch.full((1, 3, kw["canvas_h"], kw["canvas_w"]), GREY)
    out[:, :, dy0:dy0 + dh, dx0:dx0 + dw] = a * c + (1 - a) * GREY
    return out.permute(0, 2, 3, 1)


def check_premultiplied(compose):
    """compose(fg, alpha, return_placement=True, **kw) -> (out, place): no pixel is redder than the grey, although the straight resample is."""
    fg, alpha, kw = premult_scene()
    out, place = compose(fg, alpha, return_placement=True, **kw)
    out, place = out.cpu(), place.cpu()
    assert place.tolist() == [[4, 4, 32, 32, 2, 2, 16, 16]], place.tolist()
    assert float(out[..., 0].max()) <= GREY + TOL, float(out[..., 0].max())
    assert float((out - GREY).abs().max()) <= TOL
    naive = straight_resample(fg, alpha, place, kw)
    assert float(naive[..., 0].max()) > GREY + 0.02, float(naive[..., 0].max())      # the case can tell the two apart


# ---- shadow, batch, contract ------------------------------------------------------------------------------------------------------------
def check_shadow_off_is_ignored(eng, to_tensor):
    """shadow_opacity = 0: bit-identical whatever sigma and offsets are, and no blur kernel runs."""
    name, fg, alpha, kw = next(c for c in cases() if c[0] == "downscale_b2_colour_rgb")
    base = eng.compose_canvas(to_tensor(fg), to_tensor(alpha), **kw)
    eng.lib.kernel_counts(reset=True)
    for sigma, dy, dx in ((1.5, 3, -2), (32.0, -4096, 4096), (0.0, 0, 0), (float("nan"), 1, 1)):
        other = eng.compose_canvas(to_tensor(fg), to_tensor(alpha), shadow_opacity=0.0, shadow_sigma=sigma, shadow_dy=dy, shadow_dx=dx, **kw)
        assert torch.equal(base, other), (sigma, dy, dx)
    counts = eng.lib.kernel_counts()
    assert counts == {k: 4 for k in PLAIN_KERNELS}, counts
    on = eng.compose_canvas(to_tensor(fg), to_tensor(alpha), shadow_opacity=0.5, shadow_sigma=1.5, shadow_dy=3, shadow_dx=-2, **kw)
    assert float((on - base).max()) <= TOL and float((base - on).max()) > 0.05         # a black shadow only darkens


def check_transparent_shadow(eng, to_tensor):
    """On a transparent canvas the shadow shows in the alpha: A = A_s + (1 - A_s) S >= A_s, and above 0 where the subject is absent."""
    name, fg, alpha, kw = next(c for c in cases() if c[0] == "shadow_transparent")
    plain = eng.compose_canvas(to_tensor(fg), to_tensor(alpha), **{k: v for k, v in kw.items() if not k.startswith("shadow_")}).cpu()
    got = eng.compose_canvas(to_tensor(fg), to_tensor(alpha), **kw).cpu()
    As, A = plain[..., 3], got[..., 3]
    assert float((As - A).max()) <= TOL and bool(((As == 0) & (A > 0.01)).any())
    only_shadow = (As == 0) & (A > 0)
    assert bool((got[..., :3][only_shadow] == 0).all())                                # the shadow's colour is black


def check_batch_independence(eng, to_tensor):
    """Image 0 of a B = 2 call equals the B = 1 call bit for bit, with and without a shadow, 3 and 4 channels."""
    for nm in ("downscale_b2_rgba", "odd_canvas_rgb_runs", "shadow_image_rgb_odd_canvas", "shadow_transparent"):
        name, fg, alpha, kw = next(c for c in cases() if c[0] == nm)
        both, pb = eng.compose_canvas(to_tensor(fg), to_tensor(alpha), return_placement=True, **_dev_kw(kw, to_tensor))
        kw1 = dict(kw)
        if kw.get("bg_image") is not None:
            kw1["bg_image"] = kw["bg_image"][:1]
        one, p1 = eng.compose_canvas(to_tensor(fg[:1].contiguous()), to_tensor(alpha[:1].contiguous()), return_placement=True, **_dev_kw(kw1, to_tensor))
        assert torch.equal(both[:1], one) and torch.equal(pb[:1], p1), nm
        assert pb[0].tolist() != pb[1].tolist(), nm


def check_launch_counts_do_not_depend_on_input(eng, to_tensor):
    """24 x 20 and 37 x 53, empty and full alpha, B = 1 and 2: the same launches."""
    for shadow, want in ((0.0, PLAIN_KERNELS), (0.5, SHADOW_KERNELS)):
        for B, H, W, fill in ((1, 24, 20, 0.0), (1, 37, 53, 0.0), (2, 37, 53, 1.0), (1, 24, 20, 1.0)):
            eng.lib.kernel_counts(reset=True)
            eng.compose_canvas(to_tensor(torch.rand(B, H, W, 3)), to_tensor(torch.full((B, H, W), fill)), 32, 48, shadow_opacity=shadow, shadow_sigma=2.0)
            assert eng.lib.kernel_counts() == {k: 1 for k in want}, (shadow, B, H, W, fill)


def check_errors(eng, to_tensor):
    """Python raises ValueError; every invalid argument of the raw C call returns SDM_ERR_INVALID (-1) and leaves sentinel-filled outputs untouched."""
    import ctypes
    import pytest
    from comfyui_sdmatte_amd.engine import _ptr
    B, H, W, CH, CW = 1, 12, 10, 16, 20
    fg, alpha = to_tensor(torch.rand(B, H, W, 3)), to_tensor(torch.rand(B, H, W))
    bgi = to_tensor(torch.rand(1, CH, CW, 3))
    for bad in (dict(fill_pct=0), dict(fill_pct=101), dict(fill_pct=2.5), dict(valign=3), dict(valign="middle"), dict(canvas_h=0), dict(canvas_w=40000),
                dict(roi_threshold=1.0), dict(roi_threshold=float("nan")), dict(shadow_opacity=1.5), dict(shadow_opacity=-0.1),
                dict(shadow_opacity=float("nan")), dict(shadow_opacity=0.5, shadow_sigma=0.0), dict(shadow_opacity=0.5, shadow_sigma=32.5),
                dict(shadow_opacity=0.5, shadow_sigma=float("inf")), dict(shadow_dy=4097), dict(shadow_dx=-4097), dict(out_channels=3), dict(out_channels=5),
                dict(bg_color=(1.0, 0.5)), dict(bg_image=bgi[:, :5])):
        with pytest.raises(ValueError):
            eng.compose_canvas(fg, alpha, **dict(dict(canvas_h=CH, canvas_w=CW), **bad))
    with pytest.raises(ValueError):
        eng.compose_canvas(fg[..., :2], alpha, CH, CW)
    with pytest.raises(ValueError):
        eng.compose_canvas(fg, alpha[:, :5], CH, CW)
    with pytest.raises(ValueError):
        eng.compose_canvas(fg, alpha, CH, CW, out=torch.empty(B, CH, CW, 3, device=fg.device))
    out = torch.full((B, CH, CW, 4), -7.0, device=fg.device)
    place = torch.full((B, 8), -7, dtype=torch.int32, device=fg.device)
    rgb = (ctypes.c_float * 3)(0.1, 0.2, 0.3)
    kind = eng._kind(fg)
    good = dict(B=B, H=H, W=W, thr=0.0, ch=CH, cw=CW, fill=80, valign=1, bg_mode=1, rgb=rgb, bgi=None, bg_batch=0, op=0.5, sigma=2.0, dy=1, dx=1, chn=4, kind=kind)

    def raw(**kw):
        a = dict(good, **kw)
        return eng.lib.sdm_compose_canvas(eng.h, _ptr(fg), _ptr(alpha), a["B"], a["H"], a["W"], a["thr"], a["ch"], a["cw"], a["fill"], a["valign"], a["bg_mode"],
                                          a["rgb"], _ptr(a["bgi"]), a["bg_batch"], a["op"], a["sigma"], a["dy"], a["dx"], _ptr(out), a["chn"], _ptr(place),
                                          a["kind"], None)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(B=0), dict(H=0), dict(W=40000), dict(thr=1.0), dict(thr=-0.1), dict(thr=nan), dict(ch=0), dict(cw=0), dict(ch=32769), dict(ch=32768, cw=32768),
                dict(fill=0), dict(fill=101), dict(valign=-1), dict(valign=3), dict(bg_mode=-1), dict(bg_mode=3), dict(bg_mode=0, chn=3), dict(bg_mode=1, rgb=None),
                dict(bg_mode=2), dict(bg_mode=2, bgi=bgi, bg_batch=2), dict(bg_mode=2, bgi=bgi, bg_batch=0), dict(chn=2), dict(chn=5), dict(op=-0.5), dict(op=1.5),
                dict(op=nan), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=32.5), dict(sigma=nan), dict(sigma=inf), dict(dy=4097), dict(dy=-4097), dict(dx=4097),
                dict(dx=-4097), dict(kind=7)):
        assert raw(**bad) == -1, bad
        assert eng.lib.sdm_last_error(eng.h), bad
    eng.synchronize()
    assert bool((out == -7).all()) and bool((place == -7).all())
    assert raw() == 0 and raw(op=0.0, sigma=nan) == 0 and raw(bg_mode=2, bgi=bgi, bg_batch=1, chn=3) == 0      # (the last one fills 3/4 of `out`)
    eng.synchronize()
    assert not bool((place == -7).any())
