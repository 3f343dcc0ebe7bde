"""CPU-only checks of the foreground-estimation feature's host side: the torch restatement `estimate_foreground` against the numpy reference of
tests/foreground_suite.py, the recovery of a known foreground, the opt-in node surface and the exported product call."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _cpu_estimate(image, alpha, params, rgba):
    from comfyui_sdmatte_amd.sdmatte_nodes import estimate_foreground
    fg, bg, a = estimate_foreground(image, alpha, **params)
    return (torch.cat([fg, a.unsqueeze(-1)], -1) if rgba else fg), bg


def test_estimate_foreground_restatement_equals_reference(pkg):
    """Every case of the list (sizes from 1x1 to several tiles, soft / hard / constant / noise / NaN-sprinkled alpha, the parameter variants)."""
    import foreground_suite as FS
    names = [c[0] for c in FS.cases()]
    assert len(names) == len(FS.SIZES) * len(FS.PATTERNS) + 2 * len(FS.VARIANTS) and len(set(names)) == len(names)
    FS.check(_cpu_estimate, lambda t: t)


def test_reference_levels_and_resampling_by_hand(pkg):
    """The level list and the nearest index of the definition, on sizes small enough to check by eye."""
    import foreground_suite as FS
    assert FS.level_sizes(5, 300) == [(5, 300), (3, 150), (2, 75), (1, 38), (1, 19), (1, 10), (1, 5), (1, 3), (1, 2), (1, 1)]
    assert FS.n_large_levels(1024, 1024) == 5 and FS.n_large_levels(1080, 1920) == 6 and FS.n_large_levels(33, 70) == 2
    assert [FS.n_large_levels(*s) for s in ((32, 32), (1, 1), (5, 7))] == [0, 0, 0]
    assert FS._src(3, 5).tolist() == [0, 1, 3] and FS._src(5, 3).tolist() == [0, 0, 1, 1, 2] and FS._src(4, 4).tolist() == [0, 1, 2, 3]
    # alpha = 1 everywhere: the foreground is the image itself, whatever the background does
    img = np.random.default_rng(0).uniform(size=(1, 9, 11, 3)).astype(np.float32)
    fg, _ = FS.reference(img, np.ones((1, 9, 11), np.float32))
    assert np.abs(fg - img).max() < 1e-4


@pytest.mark.parametrize("H,W", [(97, 131), (64, 64), (33, 70)])
def test_estimate_foreground_recovers_a_known_foreground(pkg, H, W):
    """On the smooth composite, over the pixels with 0.05 < alpha < 1, the estimate is within 0.05 of the true foreground and at least ten times
    closer to it than the input image (whose colours carry the old background)."""
    import foreground_suite as FS
    from comfyui_sdmatte_amd.sdmatte_nodes import estimate_foreground
    image, alpha, F, _ = FS.scene(H + W, 2, H, W)
    fg, _, _ = estimate_foreground(torch.from_numpy(image), torch.from_numpy(alpha))
    sel = (alpha > 0.05) & (alpha < 1.0)
    assert sel.sum() > 50
    err = float(np.abs(fg.numpy() - F)[sel].max())
    err_image = float(np.abs(image - F)[sel].max())
    print(f"[foreground] recovery {H}x{W}: fg {err:.4f} image {err_image:.4f}")
    assert err < 0.05 and err < 0.1 * err_image, (err, err_image)


def test_estimate_foreground_argument_checks(pkg):
    from comfyui_sdmatte_amd.sdmatte_nodes import estimate_foreground
    img, a = torch.rand(1, 6, 7, 3), torch.rand(1, 6, 7)
    for bad in ({"regularization": 0.0}, {"regularization": -1e-5}, {"regularization": float("nan")}, {"gradient_weight": -0.1}, {"n_small_iters": 0},
                {"n_small_iters": 65}, {"n_big_iters": 0}, {"n_big_iters": 5}, {"n_big_iters": 1.5}):
        with pytest.raises(ValueError):
            estimate_foreground(img, a, **bad)
    with pytest.raises(ValueError):
        estimate_foreground(img[..., :2], a)
    with pytest.raises(ValueError):
        estimate_foreground(img, a[:, :5])
    estimate_foreground(img, a, regularization=1e-9, gradient_weight=0.0, n_small_iters=64, n_big_iters=4)


def test_node_mappings_with_foreground(pkg):
    """node_mappings(False) / node_mappings(True) are what they were; foreground=True adds exactly SDMatteForeground."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    classes, names = N.node_mappings(False)
    assert classes == {"SDMatteApply": N.SDMatteApply} and names == {"SDMatteApply": "Apply SDMatte"}
    classes, names = N.node_mappings(True)
    assert classes == {"SDMatteApply": N.SDMatteApply, "SDMatteTrimapFromMask": N.SDMatteTrimapFromMask, "SDMatteApplyMask": N.SDMatteApplyMask}
    assert names == {"SDMatteApply": "Apply SDMatte", "SDMatteTrimapFromMask": "SDMatte Trimap From Mask", "SDMatteApplyMask": "Apply SDMatte (Mask)"}
    for extra in (False, True):
        base_c, base_n = N.node_mappings(extra)
        assert N.node_mappings(extra, foreground=False) == (base_c, base_n)
        classes, names = N.node_mappings(extra, foreground=True)
        assert classes == dict(base_c, SDMatteForeground=N.SDMatteForeground)
        assert set(names) == set(classes) and {k: names[k] for k in base_n} == base_n
    f = N.SDMatteForeground
    it = f.INPUT_TYPES()
    assert list(it) == ["required", "optional"] and list(it["required"]) == ["image", "alpha"]
    assert it["required"]["image"][0] == "IMAGE" and it["required"]["alpha"][0] == "MASK"
    assert list(it["optional"]) == ["regularization", "gradient_weight", "n_small_iters", "n_big_iters"]
    reg, gw, ns, nb = (it["optional"][k] for k in it["optional"])
    assert reg[0] == "FLOAT" and reg[1]["default"] == 1e-5 and reg[1]["min"] > 0
    assert gw[0] == "FLOAT" and gw[1]["default"] == 1.0 and gw[1]["min"] == 0.0
    assert ns[0] == "INT" and (ns[1]["default"], ns[1]["min"], ns[1]["max"]) == (10, 1, 64)
    assert nb[0] == "INT" and (nb[1]["default"], nb[1]["min"], nb[1]["max"]) == (2, 1, 4)
    assert f.RETURN_TYPES == ("IMAGE", "IMAGE", "IMAGE") and f.RETURN_NAMES == ("foreground", "background", "foreground_rgba")
    assert f.CATEGORY == "Matting/SDMatte" and callable(getattr(f, f.FUNCTION))
    import inspect
    assert list(inspect.signature(getattr(f, f.FUNCTION)).parameters) == ["self", "image", "alpha", "regularization", "gradient_weight", "n_small_iters",
                                                                           "n_big_iters"]
    with pytest.raises(ValueError):
        f().estimate(torch.zeros(1, 8, 8, 4), torch.zeros(1, 8, 8))
    with pytest.raises(ValueError):
        f().estimate(torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 7))


def test_foreground_node_env_opt_in(pkg):
    """The module-level mappings follow SDMATTE_FOREGROUND_NODE, independently of SDMATTE_EXTRA_NODES: a fresh interpreter each."""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; p = load_package(); "
            "print(sorted(p.NODE_CLASS_MAPPINGS), sorted(p.NODE_DISPLAY_NAME_MAPPINGS))" % ROOT)
    base = "['SDMatteApply']"
    both = "['SDMatteApply', 'SDMatteApplyMask', 'SDMatteTrimapFromMask']"
    fgn = "['SDMatteApply', 'SDMatteForeground']"
    allx = "['SDMatteApply', 'SDMatteApplyMask', 'SDMatteForeground', 'SDMatteTrimapFromMask']"
    for extra, fgv, want in ((None, None, base), ("1", "0", both), (None, "1", fgn), ("1", "1", allx)):
        env = {k: v for k, v in os.environ.items() if k not in ("SDMATTE_EXTRA_NODES", "SDMATTE_FOREGROUND_NODE")}
        if extra is not None:
            env["SDMATTE_EXTRA_NODES"] = extra
        if fgv is not None:
            env["SDMATTE_FOREGROUND_NODE"] = fgv
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.strip() == f"{want} {want}", (extra, fgv, r.stdout, r.stderr)


def test_product_library_exports_estimate_foreground(pkg):
    """The gfx950 library exports the new product call, the header carries the defaults and limits, and the bindings mirror them."""
    from comfyui_sdmatte_amd import build, engine
    dll = ctypes.CDLL(build.build_all())
    assert "sdm_estimate_foreground" in engine.EXPORTS
    getattr(dll, "sdm_estimate_foreground")
    hdr = open(os.path.join(ROOT, "include", "sdmatte.h")).read()
    E = engine.Engine
    for line in ("#define SDM_FG_REGULARIZATION 1e-5f", "#define SDM_FG_GRADIENT_WEIGHT 1.0f", f"#define SDM_FG_SMALL_ITERS {E.FG_DEFAULTS['n_small_iters']}",
                 f"#define SDM_FG_BIG_ITERS {E.FG_DEFAULTS['n_big_iters']}", f"#define SDM_FG_MAX_SMALL_ITERS {E.FG_MAX_SMALL_ITERS}",
                 f"#define SDM_FG_MAX_BIG_ITERS {E.FG_MAX_BIG_ITERS}", f"#define SDM_FG_MAX_SIDE {E.FG_MAX_SIDE}", f"#define SDM_FG_MAX_PIXELS {E.FG_MAX_PIXELS}"):
        assert line in hdr, line
    assert E.FG_DEFAULTS["regularization"] == 1e-5 and E.FG_DEFAULTS["gradient_weight"] == 1.0
