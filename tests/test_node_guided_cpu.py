"""CPU-only checks of the guided alpha refinement's host side: the torch restatement `guided_refine_alpha` against the numpy reference of
tests/guided_suite.py, what the call is for (a blurred 2-pixel edge comes back), `auto_subsample`, the opt-in node surface and the exported call."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def test_guided_refine_alpha_restatement_equals_reference(pkg):
    """Every case of the list: each size (1x1 to several tiles) with each (subsample, radius, eps) triple - s not dividing H or W, a coarse grid of 1x1,
    windows larger than the grid, the largest radius, the smallest eps - and every alpha pattern."""
    import guided_suite as GS
    from comfyui_sdmatte_amd.sdmatte_nodes import guided_refine_alpha
    names = [c[0] for c in GS.cases()]
    assert len(names) == len(GS.SIZES) * len(GS.TRIPLES) and len(set(names)) == len(names)
    assert {n.split("_")[0] for n in names} == set(GS.PATTERNS)
    GS.check(guided_refine_alpha, lambda t: t)


def test_reference_by_hand(pkg):
    """Pieces of the definition on inputs small enough to check by eye."""
    import guided_suite as GS
    x = np.arange(10, dtype=np.float64).reshape(1, 10)
    acc, cnt = GS._block_sum(x, 1, 4, 3)
    assert acc.tolist() == [[0 + 1 + 2 + 3, 4 + 5 + 6 + 7, 8 + 9]] and cnt.tolist() == [4, 4, 2]
    acc, cnt = GS._window_sum(x[:, :4], 1, 2)
    assert acc.tolist() == [[3, 6, 6, 6]] and cnt.tolist() == [3, 4, 4, 3]
    i0, i1, f = GS._upsample_axis(8, 2, 4, np.float64)
    assert i0.tolist() == [0] * 6 + [1, 1] and i1.tolist() == [1] * 8
    assert np.allclose(f, [0, 0, 0.125, 0.375, 0.625, 0.875, 0, 0])
    # alpha = a0 . I + b0 exactly: the fit finds it (eps small) and the call returns it, whatever the subsample
    rng = np.random.default_rng(0)
    img = rng.uniform(size=(1, 24, 30, 3)).astype(np.float32)
    alpha = (img * np.array([0.2, 0.3, 0.1])).sum(-1) + 0.2
    for s in (1, 2):
        assert np.abs(GS.reference(img, alpha, s, 3, 1e-6) - alpha).max() < 2e-4
    # a constant alpha stays what it is
    assert np.abs(GS.reference(img, np.full((1, 24, 30), 0.25, np.float32), 4, 2, 1e-4) - 0.25).max() < 1e-12


def test_guided_refine_alpha_serves_its_purpose(pkg):
    """A composite with a 2-pixel edge whose alpha went through a reduction by 4: refined with subsample 4 the max error is at most half the bilinear
    alpha's and the mean error no larger - on the reference in fp64 and on the restatement.  With subsample 1 (the classic filter on the blurred alpha)
    nothing of that kind happens, which is why the parameter exists."""
    import guided_suite as GS
    from comfyui_sdmatte_amd.sdmatte_nodes import guided_refine_alpha
    image, true, blurred = GS.purpose_scene()
    assert image.shape == (1, 256, 384, 3) and float(np.abs(blurred - true).max()) > 0.3
    GS.check_purpose(GS.reference(image, blurred, *GS.PURPOSE), "reference, fp64")
    GS.check_purpose(guided_refine_alpha(torch.from_numpy(image), torch.from_numpy(blurred), *GS.PURPOSE).numpy(), "restatement")
    classic = GS.reference(image, blurred, 1, GS.PURPOSE[1], GS.PURPOSE[2])
    assert np.abs(classic - true).max() > 0.5 * np.abs(blurred - true).max()


def test_auto_subsample(pkg):
    from comfyui_sdmatte_amd.sdmatte_nodes import auto_subsample
    for (H, W, S), want in {(2160, 3840, 1024): 4, (3840, 2160, 1024): 4, (1024, 1024, 1024): 1, (1025, 600, 1024): 2, (512, 300, 1024): 1, (2048, 2048, 512): 4,
                            (1, 1, 512): 1, (20000, 100, 512): 16, (8192, 8193, 512): 16, (8192, 8192, 512): 16, (7680, 100, 512): 15, (2049, 5, 1024): 3}.items():
        assert auto_subsample(H, W, S) == want, (H, W, S)
    for bad in ((0, 5, 512), (5, 5, 0)):
        with pytest.raises(ValueError):
            auto_subsample(*bad)


def test_guided_refine_alpha_argument_checks(pkg):
    from comfyui_sdmatte_amd.sdmatte_nodes import guided_refine_alpha
    img, a = torch.rand(1, 6, 7, 3), torch.rand(1, 6, 7)
    for bad in ({"subsample": 0}, {"subsample": 17}, {"subsample": 1.5}, {"radius": 0}, {"radius": 33}, {"eps": 0.0}, {"eps": 5e-7}, {"eps": 1.5},
                {"eps": float("nan")}, {"eps": float("inf")}):
        with pytest.raises(ValueError):
            guided_refine_alpha(img, a, **dict({"subsample": 2}, **bad))
    with pytest.raises(ValueError):
        guided_refine_alpha(img[..., :2], a, 2)
    with pytest.raises(ValueError):
        guided_refine_alpha(img, a[:, :5], 2)
    with pytest.raises(ValueError):
        guided_refine_alpha(img[0], a[0], 2)
    for good in ({"subsample": 16, "radius": 32, "eps": 1.0}, {"subsample": 1, "radius": 1, "eps": 1e-6}, {"subsample": 2, "eps": float(np.float32(1e-6))}):
        out = guided_refine_alpha(img, a, **good)
        assert out.shape == a.shape and out.dtype == torch.float32


def test_node_mappings_with_refine(pkg):
    """The default mappings and the two earlier flags are what they were; refine=True adds exactly SDMatteRefineAlpha."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    classes, names = N.node_mappings(False)
    assert classes == {"SDMatteApply": N.SDMatteApply} and names == {"SDMatteApply": "Apply SDMatte"}
    for extra in (False, True):
        for fg in (False, True):
            base_c, base_n = N.node_mappings(extra, fg)
            assert N.node_mappings(extra, fg, False) == (base_c, base_n) == N.node_mappings(extra, foreground=fg, refine=False)
            classes, names = N.node_mappings(extra, fg, refine=True)
            assert classes == dict(base_c, SDMatteRefineAlpha=N.SDMatteRefineAlpha)
            assert names == dict(base_n, SDMatteRefineAlpha="SDMatte Refine Alpha")
    f = N.SDMatteRefineAlpha
    it = f.INPUT_TYPES()
    assert list(it) == ["required", "optional"] and list(it["required"]) == ["image", "alpha", "inference_size"]
    assert it["required"]["image"][0] == "IMAGE" and it["required"]["alpha"][0] == "MASK"
    assert it["required"]["inference_size"] == N.SDMatteApply.INPUT_TYPES()["required"]["inference_size"]
    assert it["required"]["inference_size"][1]["default"] == 1024
    assert list(it["optional"]) == ["subsample", "radius", "eps"]
    sub, rad, eps = (it["optional"][k] for k in it["optional"])
    assert sub[0] == "INT" and (sub[1]["default"], sub[1]["min"], sub[1]["max"]) == (0, 0, 16)
    assert rad[0] == "INT" and (rad[1]["default"], rad[1]["min"], rad[1]["max"]) == (2, 1, 32)
    assert eps[0] == "FLOAT" and (eps[1]["default"], eps[1]["min"], eps[1]["max"]) == (1e-4, 1e-6, 1.0)
    assert f.RETURN_TYPES == ("MASK", ) and f.RETURN_NAMES == ("alpha_mask", )
    assert f.CATEGORY == "Matting/SDMatte" and callable(getattr(f, f.FUNCTION))
    import inspect
    assert list(inspect.signature(getattr(f, f.FUNCTION)).parameters) == ["self", "image", "alpha", "inference_size", "subsample", "radius", "eps"]
    with pytest.raises(ValueError):
        f().refine(torch.zeros(1, 8, 8, 4), torch.zeros(1, 8, 8))
    with pytest.raises(ValueError):
        f().refine(torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 7))


def test_refine_node_env_opt_in(pkg):
    """The module-level mappings follow SDMATTE_REFINE_NODE, independently of the other two flags: a fresh interpreter each."""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; p = load_package(); "
            "print(sorted(p.NODE_CLASS_MAPPINGS), sorted(p.NODE_DISPLAY_NAME_MAPPINGS))" % ROOT)
    flags = ("SDMATTE_EXTRA_NODES", "SDMATTE_FOREGROUND_NODE", "SDMATTE_REFINE_NODE")
    for extra, fgv, ref, want in ((None, None, None, "['SDMatteApply']"), (None, None, "0", "['SDMatteApply']"),
                                  (None, None, "1", "['SDMatteApply', 'SDMatteRefineAlpha']"),
                                  ("1", "1", "1", "['SDMatteApply', 'SDMatteApplyMask', 'SDMatteForeground', 'SDMatteRefineAlpha', 'SDMatteTrimapFromMask']")):
        env = {k: v for k, v in os.environ.items() if k not in flags}
        env.update({k: v for k, v in zip(flags, (extra, fgv, ref)) if v is not None})
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.strip() == f"{want} {want}", (extra, fgv, ref, r.stdout, r.stderr)


def test_product_library_exports_refine_alpha_guided(pkg):
    """The gfx950 library exports the new product call, the header carries the defaults and limits, and the bindings mirror them."""
    from comfyui_sdmatte_amd import build, engine
    dll = ctypes.CDLL(build.build_all())
    assert "sdm_refine_alpha_guided" in engine.EXPORTS
    getattr(dll, "sdm_refine_alpha_guided")
    hdr = open(os.path.join(ROOT, "include", "sdmatte.h")).read()
    E = engine.Engine
    for line in (f"#define SDM_GF_RADIUS {E.GF_DEFAULTS['radius']}", "#define SDM_GF_EPS 1e-4f", f"#define SDM_GF_MAX_SUBSAMPLE {E.GF_MAX_SUBSAMPLE}",
                 f"#define SDM_GF_MAX_RADIUS {E.GF_MAX_RADIUS}"):
        assert line in hdr, line
    assert E.GF_DEFAULTS["eps"] == 1e-4 and (E.GF_MAX_SUBSAMPLE, E.GF_MAX_RADIUS) == (16, 32)
