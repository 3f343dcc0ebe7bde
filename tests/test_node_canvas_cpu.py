"""CPU-only checks of the canvas call's host side: `canvas_fit` against the definition in Python integers, the measurement behind the tolerance of
tests/canvas_suite.py, the torch restatement `compose_canvas` on inputs small enough to check by hand, the opt-in node and the exported call."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def test_canvas_fit_by_hand(pkg):
    from comfyui_sdmatte_amd.sdmatte_nodes import canvas_fit
    # a tall box on a wide canvas: the height decides; 80 % of 100 = 80 rows, 20 * 80 / 40 = 40 columns
    assert canvas_fit([[3, 4, 40, 20]], 100, 200, 80, "center").tolist() == [[3, 4, 40, 20, 10, 80, 80, 40]]
    # a wide box: the width decides; 160 columns, (10 * 160 + 20) / 40 = 40 rows; top = margin 10, centre 30, bottom 100 - 10 - 40 = 50
    for valign, dy0 in (("top", 10), ("center", 30), ("bottom", 50), (0, 10), (1, 30), (2, 50)):
        assert canvas_fit([[0, 0, 10, 40]], 100, 200, 80, valign).tolist() == [[0, 0, 10, 40, dy0, 20, 40, 160]]
    # rounding to nearest: 7 x 3 into 10 x 10 at 100 %: dw = (3 * 10 + 3) / 7 = 4; fill_pct 1 on a small canvas: one pixel
    assert canvas_fit([[0, 0, 7, 3]], 10, 10, 100, 1).tolist() == [[0, 0, 7, 3, 0, 3, 10, 4]]
    assert canvas_fit([[0, 0, 7, 3]], 10, 10, 1, 2).tolist() == [[0, 0, 7, 3, 5, 4, 1, 1]]            # mv = 4: 10 - 4 - 1
    # a very thin box keeps one pixel; 64-bit products
    assert canvas_fit([[0, 0, 1000, 1]], 10, 10, 100, 1)[0, 6:].tolist() == [10, 1]
    big = canvas_fit([[0, 0, 32768, 32767]], 16384, 16384, 100, 1)[0].tolist()
    assert big[4:] == [0, 0, 16384, 16384]
    assert canvas_fit(torch.tensor([[0, 0, 5, 5], [1, 1, 2, 8]]), 20, 20).dtype == torch.int32
    for bad in (dict(fill_pct=0), dict(fill_pct=101), dict(valign=3), dict(valign="middle"), dict(canvas_h=0), dict(canvas_w=32769)):
        with pytest.raises(ValueError):
            canvas_fit([[0, 0, 5, 5]], **dict(dict(canvas_h=10, canvas_w=10), **bad))
    with pytest.raises(ValueError):
        canvas_fit([[0, 0, 0, 5]], 10, 10)


def test_canvas_cases_mean_what_their_names_say(pkg):
    """Both branches of the fit, the copy branch, every (fill_pct, valign) pair, boxes at the frame edge and different boxes in a batch are in the list."""
    import canvas_suite as CS
    cases = {c[0]: c for c in CS.cases()}
    assert len(cases) == len(CS.cases())
    place = {n: CS.reference64(c)[1] for n, c in cases.items()}
    p = place["copy_branch"][0].tolist()
    assert p[2:4] == p[6:8] == [20, 16]
    p = place["downscale_b2_rgba"].tolist()
    assert p[0] != p[1] and all(q[6] < q[2] and q[7] < q[3] for q in p)
    p = place["upscale_fill100"][0].tolist()
    assert p[6] > p[2] and p[7] > p[3] and (p[6] == 64 or p[7] == 40)
    assert place["empty_alpha"][0].tolist()[:4] == [0, 0, 24, 20]
    p = place["edge_box"][0].tolist()
    assert p[0] == 0 and p[1] + p[3] == 53
    seen = set()
    for n, c in cases.items():
        if n.startswith("fit_") and "fill" in n:
            q = place[n][0].tolist()
            th, tw = max(1, 32 * c[3]["fill_pct"] // 100), max(1, 48 * c[3]["fill_pct"] // 100)
            assert (q[6] == th) == ("tall" in n) and (q[7] == tw) == ("wide" in n) or th == 1, (n, q)
            seen.add((c[3]["fill_pct"], c[3]["valign"]))
    assert seen == {(f, v) for f in (100, 50, 1) for v in (0, 1, 2)}
    assert place["fit_tall_square_canvas"][0, 6] == 28 and place["fit_wide_square_canvas"][0, 7] == 28
    r = 96
    assert cases["shadow_sigma32_canvas40"][3]["canvas_h"] < r


def test_tolerance_measurement(pkg):
    """The float32 restatement against the float64 one on every case: the deviation behind canvas_suite.TOL, and the share of pixels the straight-colour
    comparison leaves out."""
    import canvas_suite as CS
    worst, pos, low = 0.0, 0, 0
    for case in CS.cases():
        want, wplace = CS.reference64(case)
        got, place = CS.reference(case[1], case[2], case[3], torch.float32)
        assert torch.equal(place, wplace) and got.dtype == torch.float32 and want.dtype == torch.float64
        d, p, lo = CS.deviation(got, want)
        worst, pos, low = max(worst, d), pos + p, low + lo
    print(f"float32 against float64: {worst:.3e}; {low} of {pos} pixels with A > 0 are below 1/64")
    assert CS.TOL == 4 * CS.MEASURED_F32_DEVIATION
    assert CS.MEASURED_F32_DEVIATION / 2 <= worst <= CS.TOL, worst
    assert pos > 10000 and low <= 0.05 * pos, (low, pos)


def test_compose_canvas_by_hand(pkg):
    """One opaque pixel, copied to the middle of a 9 x 9 canvas: the layer, the shadow's weights and offset, and each background, value by value."""
    import math
    from comfyui_sdmatte_amd.sdmatte_nodes import compose_canvas
    fg, a = torch.tensor([[[[0.2, 0.4, 0.6]]]]), torch.ones(1, 1, 1)
    out, place = compose_canvas(fg, a, 9, 9, fill_pct=12, dtype=torch.float64, return_placement=True)
    assert place.tolist() == [[0, 0, 1, 1, 4, 4, 1, 1]] and out.shape == (1, 9, 9, 4) and out.dtype == torch.float64
    want = torch.zeros(1, 9, 9, 4, dtype=torch.float64)
    want[0, 4, 4] = torch.tensor([0.2, 0.4, 0.6, 1.0], dtype=torch.float32).double()
    assert torch.equal(out, want)
    sigma, op = 0.5, 0.75
    g = [math.exp(-i * i / (2 * sigma * sigma)) for i in range(-2, 3)]                # r = ceil(1.5) = 2
    w = [float(np.float32(v / sum(g))) for v in g]
    sh = compose_canvas(fg, a, 9, 9, fill_pct=12, shadow_opacity=op, shadow_sigma=sigma, shadow_dy=1, shadow_dx=-1, dtype=torch.float64)
    for y in range(9):
        for x in range(9):
            j, i = y - 1 - 4 + 2, x + 1 - 4 + 2
            S = op * w[j] * w[i] if 0 <= j < 5 and 0 <= i < 5 else 0.0
            A = 1.0 if (y, x) == (4, 4) else S
            assert abs(float(sh[0, y, x, 3]) - A) < 1e-15, (y, x)
            assert (y, x) == (4, 4) or float(sh[0, y, x, :3].abs().max()) == 0.0
    grey = compose_canvas(fg, a, 9, 9, fill_pct=12, bg_color=(0.5, 0.5, 0.5), shadow_opacity=op, shadow_sigma=sigma, shadow_dy=1, shadow_dx=-1, dtype=torch.float64)
    assert grey.shape == (1, 9, 9, 3)
    assert abs(float(grey[0, 5, 3, 0]) - 0.5 * (1 - op * w[2] * w[2])) < 1e-15 and float(grey[0, 0, 8, 0]) == 0.5
    assert torch.equal(grey[0, 4, 4], want[0, 4, 4, :3])
    img = torch.rand(1, 9, 9, 3)
    over = compose_canvas(fg, a, 9, 9, fill_pct=12, bg_image=img, out_channels=4)
    assert over.dtype == torch.float32 and bool((over[..., 3] == 1.0).all())
    assert torch.equal(over[0, 0, 0, :3], img[0, 0, 0]) and torch.equal(over[0, 4, 4, :3], fg[0, 0, 0])
    for bad in (dict(out_channels=3), dict(bg_color=(1.0, 1.0)), dict(bg_image=img[:, :5]), dict(dtype=torch.float16), dict(shadow_opacity=2.0),
                dict(shadow_opacity=0.5, shadow_sigma=40.0)):
        with pytest.raises(ValueError):
            compose_canvas(fg, a, 9, 9, **bad)


def test_compose_canvas_premultiplication_is_real(pkg):
    import canvas_suite as CS
    from comfyui_sdmatte_amd.sdmatte_nodes import compose_canvas
    CS.check_premultiplied(compose_canvas)


def test_node_mappings_with_canvas(pkg):
    """Every earlier argument combination returns what it returned; canvas=True adds exactly SDMatteCanvas."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    from comfyui_sdmatte_amd.engine import Engine
    assert N.node_mappings(False) == ({"SDMatteApply": N.SDMatteApply}, {"SDMatteApply": "Apply SDMatte"})
    for flags in ((False, False, False, False, False), (True, False, True, False, True), (True, True, True, True, True)):
        base_c, base_n = N.node_mappings(*flags)
        assert N.node_mappings(*flags, False) == (base_c, base_n) == N.node_mappings(*flags, canvas=False) and "SDMatteCanvas" not in base_c
        classes, names = N.node_mappings(*flags, canvas=True)
        assert classes == dict(base_c, SDMatteCanvas=N.SDMatteCanvas) and names == dict(base_n, SDMatteCanvas="SDMatte Canvas")
    f = N.SDMatteCanvas
    it = f.INPUT_TYPES()
    assert list(it["required"]) == ["foreground", "alpha", "canvas_width", "canvas_height"]
    assert it["required"]["foreground"][0] == "IMAGE" and it["required"]["alpha"][0] == "MASK" and it["optional"]["background_image"][0] == "IMAGE"
    assert f.RETURN_TYPES == ("IMAGE", ) and f.CATEGORY == "Matting/SDMatte"
    assert list(inspect.signature(getattr(f, f.FUNCTION)).parameters) == ["self"] + list(it["required"]) + list(it["optional"])
    # the node's defaults are the engine call's
    defaults = {k: v.default for k, v in inspect.signature(Engine.compose_canvas).parameters.items() if v.default is not inspect.Parameter.empty}
    for k in ("fill_pct", "valign", "shadow_opacity", "shadow_sigma", "shadow_dy", "shadow_dx"):
        assert it["optional"][k][1]["default"] == defaults[k], k
    assert (it["optional"]["shadow_sigma"][1]["max"], it["optional"]["shadow_dy"][1]["max"]) == (Engine.CANVAS_MAX_SHADOW_SIGMA, Engine.CANVAS_MAX_SHADOW_OFFSET)
    # input validation comes before any engine is looked for
    fg, a = torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8)
    for bad in ((fg[..., :2], a, 16, 16), (fg, a[:, :4], 16, 16), (fg, a, 0, 16), (fg, a, 16, 16, 0), (fg, a, 16, 16, 80, "middle"), (fg, a, 16, 16, 80, "top", "image")):
        with pytest.raises(ValueError):
            f().compose(*bad)
    with pytest.raises(ValueError):
        f().compose(fg, a, 16, 16, background_image=torch.zeros(1, 8, 8, 3))


def test_canvas_node_cpu_path_equals_compose_canvas(pkg):
    """force_cpu=True is the torch restatement, argument by argument (width before height at the node, as in ComfyUI)."""
    import canvas_suite as CS
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    name, fg, alpha, kw = next(c for c in CS.cases() if c[0] == "shadow_leaves_canvas_colour")
    r, g, b = kw["bg_color"]
    out, = N.SDMatteCanvas().compose(fg, alpha, kw["canvas_w"], kw["canvas_h"], kw["fill_pct"], "center", "color", r, g, b, kw["shadow_opacity"],
                                     kw["shadow_sigma"], kw["shadow_dy"], kw["shadow_dx"], force_cpu=True)
    assert torch.equal(out, N.compose_canvas(fg, alpha, **kw)) and out.shape == (2, 32, 48, 3)
    out, = N.SDMatteCanvas().compose(fg, alpha, 48, 32, background="transparent", force_cpu=True)
    assert torch.equal(out, N.compose_canvas(fg, alpha, 32, 48)) and out.shape[-1] == 4
    bg = torch.rand(1, 32, 48, 3)
    out, = N.SDMatteCanvas().compose(fg, alpha, 48, 32, valign="bottom", background_image=bg, force_cpu=True)
    assert torch.equal(out, N.compose_canvas(fg, alpha, 32, 48, valign="bottom", bg_image=bg))


def test_canvas_node_env_opt_in(pkg):
    """The module-level mappings follow SDMATTE_CANVAS_NODE, independently of the other flags: a fresh interpreter each."""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; p = load_package(); "
            "print(sorted(p.NODE_CLASS_MAPPINGS), sorted(p.NODE_DISPLAY_NAME_MAPPINGS))" % ROOT)
    flags = ("SDMATTE_EXTRA_NODES", "SDMATTE_FOREGROUND_NODE", "SDMATTE_REFINE_NODE", "SDMATTE_CLEAN_NODE", "SDMATTE_ROI_NODE", "SDMATTE_CANVAS_NODE")
    for roi, canvas, want in ((None, None, "['SDMatteApply']"), (None, "0", "['SDMatteApply']"), (None, "1", "['SDMatteApply', 'SDMatteCanvas']"),
                              ("1", "1", "['SDMatteApply', 'SDMatteApplyROI', 'SDMatteCanvas']")):
        env = {k: v for k, v in os.environ.items() if k not in flags}
        env.update({k: v for k, v in (("SDMATTE_ROI_NODE", roi), ("SDMATTE_CANVAS_NODE", canvas)) if v is not None})
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.strip() == f"{want} {want}", (roi, canvas, r.stdout, r.stderr)


def test_product_library_exports_compose_canvas(pkg):
    """The gfx950 library exports the new product call, and header and bindings agree on the limits."""
    from comfyui_sdmatte_amd import build, engine
    dll = ctypes.CDLL(build.build_all())
    assert "sdm_compose_canvas" in engine.EXPORTS
    getattr(dll, "sdm_compose_canvas")
    hdr = open(os.path.join(ROOT, "include", "sdmatte.h")).read()
    E = engine.Engine
    for line in (f"#define SDM_CANVAS_MAX_SHADOW_SIGMA {E.CANVAS_MAX_SHADOW_SIGMA}\n", f"#define SDM_CANVAS_MAX_SHADOW_RADIUS {E.CANVAS_MAX_SHADOW_RADIUS}\n",
                 f"#define SDM_CANVAS_MAX_SHADOW_OFFSET {E.CANVAS_MAX_SHADOW_OFFSET}\n"):
        assert line in hdr, line
    assert E.CANVAS_MAX_SHADOW_RADIUS == 3 * E.CANVAS_MAX_SHADOW_SIGMA
    kernels = open(os.path.join(ROOT, "comfyui-sdmatte_amd", "csrc", "k_canvas.h")).read()
    assert f"#define SDM_CANVAS_R {E.CANVAS_MAX_SHADOW_RADIUS} " in kernels
