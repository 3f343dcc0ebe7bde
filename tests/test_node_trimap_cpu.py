"""CPU-only checks of the trimap-from-mask feature's host side: the CPU restatement `trimap_from_mask` against the brute force, the two
references of tests/trimap_suite.py against each other, the opt-in node surface, and the argument checks that need no engine."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def test_trimap_from_mask_equals_brute_force(pkg):
    """The restatement the kernels are compared with, on every case of the list: blobs, thin lines, isolated pixels, objects on each border,
    all-foreground / all-background, erode != dilate, radius 0, radius larger than the image, NaN and values equal to the threshold."""
    import trimap_suite as TS
    from comfyui_sdmatte_amd.sdmatte_nodes import trimap_from_mask
    names = [c[0] for c in TS.small_cases()]
    for want in ("blobs_", "thin_lines_", "isolated_pixels_", "touching_borders_", "all_foreground_", "all_background_", "erode_ne_dilate_",
                 "radius_zero_", "radius_larger_than_image_", "nan_and_equal_to_threshold_"):
        assert any(n.startswith(want) or want in n for n in names), want
    TS.check_make_trimap(lambda m, thr, e, d: trimap_from_mask(m, thr, e, d), lambda t: t)


def test_trimap_semantics_by_hand(pkg):
    """The definition on masks small enough to check by eye: closed disk (dx^2 + dy^2 <= r^2), strict threshold, border pixels do not exist."""
    from comfyui_sdmatte_amd.sdmatte_nodes import trimap_from_mask
    m = torch.zeros(1, 9, 9)
    m[0, 4, 4] = 1.0
    t = trimap_from_mask(m, 0.5, 0, 2)[0]
    want = torch.zeros(9, 9)
    for y in range(9):
        for x in range(9):
            if (y - 4) ** 2 + (x - 4) ** 2 <= 4:
                want[y, x] = 0.5
    want[4, 4] = 1.0                                   # erode_px = 0: the pixel itself stays foreground
    assert torch.equal(t, want)
    lone = torch.zeros(9, 9)
    lone[4, 4] = 0.5                                   # dilate_px = 0, erode_px = 1: only the pixel itself turns unknown
    assert torch.equal(trimap_from_mask(m, 0.5, 1, 0)[0], lone)
    full = torch.ones(1, 6, 7)
    assert torch.equal(trimap_from_mask(full, 0.5, 255, 255), full)                       # nothing outside F exists, not even beyond the border
    assert torch.equal(trimap_from_mask(full * 0.5, 0.5, 3, 3), torch.zeros(1, 6, 7))     # equal to the threshold: background
    assert torch.equal(trimap_from_mask(full * float("nan"), 0.5, 3, 3), torch.zeros(1, 6, 7))
    half = torch.zeros(1, 8, 8)
    half[0, :, :4] = 1.0                               # object cut by the frame on three sides: definite foreground up to the edge
    t = trimap_from_mask(half, 0.5, 2, 1)[0]
    assert torch.equal(t[:, :2], torch.ones(8, 2)) and torch.equal(t[:, 2:5], torch.full((8, 3), 0.5)) and torch.equal(t[:, 5:], torch.zeros(8, 3))
    soft = torch.rand(2, 11, 13, generator=torch.Generator().manual_seed(1))
    assert torch.equal(trimap_from_mask(soft, 0.4, 0, 0), (soft > 0.4).float())            # radii 0: the binarised mask
    for bad in ((-1, 3), (3, 256), (2.5, 3)):
        with pytest.raises(ValueError):
            trimap_from_mask(soft, 0.5, *bad)


def test_separable_reference_equals_brute_force(pkg):
    """The larger GPU cases are compared with the separable numpy reference: here it is proven equal to the brute force on every small case."""
    import trimap_suite as TS
    for name, mask, thr, e, d in TS.small_cases():
        assert np.array_equal(TS.separable(mask, thr, e, d), TS.brute_force(mask, thr, e, d)), name


def test_node_mappings_default_and_extra(pkg):
    """The default node surface is the reference's; SDMATTE_EXTRA_NODES=1 adds exactly the two mask nodes."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    classes, names = N.node_mappings(False)
    assert classes == {"SDMatteApply": N.SDMatteApply} and names == {"SDMatteApply": "Apply SDMatte"}
    classes, names = N.node_mappings(True)
    assert classes == {"SDMatteApply": N.SDMatteApply, "SDMatteTrimapFromMask": N.SDMatteTrimapFromMask, "SDMatteApplyMask": N.SDMatteApplyMask}
    assert set(names) == set(classes) and names["SDMatteApply"] == "Apply SDMatte"
    if os.environ.get("SDMATTE_EXTRA_NODES") != "1":
        assert N.NODE_CLASS_MAPPINGS == {"SDMatteApply": N.SDMatteApply}
    t = N.SDMatteTrimapFromMask
    it = t.INPUT_TYPES()
    assert list(it) == ["required"] and list(it["required"]) == ["mask", "threshold", "erode_px", "dilate_px"]
    assert it["required"]["mask"][0] == "MASK" and it["required"]["threshold"][0] == "FLOAT" and it["required"]["threshold"][1]["default"] == 0.5
    for k in ("erode_px", "dilate_px"):
        spec = it["required"][k]
        assert spec[0] == "INT" and (spec[1]["default"], spec[1]["min"], spec[1]["max"]) == (10, 0, 255)
    assert t.RETURN_TYPES == ("MASK",) and t.RETURN_NAMES == ("trimap",) and t.CATEGORY == "Matting/SDMatte" and callable(getattr(t, t.FUNCTION))
    a = N.SDMatteApplyMask
    base, it = N.SDMatteApply.INPUT_TYPES(), a.INPUT_TYPES()
    want = []
    for k in base["required"]:
        want += ["mask", "threshold", "erode_px", "dilate_px"] if k == "trimap" else [k]
    assert list(it["required"]) == want and it["optional"] == base["optional"] and "trimap" not in it["required"]
    for k in base["required"]:
        if k != "trimap":
            assert it["required"][k] == base["required"][k]
    assert it["required"]["mask"][0] == "MASK" and it["required"]["erode_px"] == N.SDMatteTrimapFromMask.INPUT_TYPES()["required"]["erode_px"]
    assert a.RETURN_TYPES == ("MASK", "IMAGE", "MASK") and a.RETURN_NAMES == ("alpha_mask", "matted_image", "trimap")
    assert a.CATEGORY == "Matting/SDMatte" and callable(getattr(a, a.FUNCTION))
    import inspect
    assert list(inspect.signature(a.apply_matte).parameters) == ["self", "ckpt_name", "image", "mask", "threshold", "erode_px", "dilate_px", "inference_size",
                                                                 "is_transparent", "output_mode", "mask_refine", "trimap_constraint", "force_cpu"]
    with pytest.raises(RuntimeError):
        a().apply_matte("SDMatte.safetensors", torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8), 0.5, 10, 10, 512, False, "alpha_only", True, 0.8, force_cpu=True)


def test_extra_nodes_env_opt_in(pkg):
    """The module-level mappings follow SDMATTE_EXTRA_NODES (read at import, like SDMATTE_MULTI_GPU is read at call time): a fresh interpreter each."""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; p = load_package(); "
            "print(sorted(p.NODE_CLASS_MAPPINGS), sorted(p.NODE_DISPLAY_NAME_MAPPINGS))" % ROOT)
    for val, want in ((None, "['SDMatteApply'] ['SDMatteApply']"), ("0", "['SDMatteApply'] ['SDMatteApply']"),
                      ("1", "['SDMatteApply', 'SDMatteApplyMask', 'SDMatteTrimapFromMask'] ['SDMatteApply', 'SDMatteApplyMask', 'SDMatteTrimapFromMask']")):
        env = {k: v for k, v in os.environ.items() if k != "SDMATTE_EXTRA_NODES"}
        if val is not None:
            env["SDMATTE_EXTRA_NODES"] = val
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.strip() == want, (val, r.stdout, r.stderr)


def test_product_library_exports_trimap_calls(pkg):
    """The gfx950 library exports the two new product calls with the header's radius bound, and the bindings name them."""
    from comfyui_sdmatte_amd import build, engine
    dll = ctypes.CDLL(build.build_all())
    for name in ("sdm_make_trimap", "sdm_apply_matte_mask"):
        assert name in engine.EXPORTS
        getattr(dll, name)
    hdr = open(os.path.join(ROOT, "include", "sdmatte.h")).read()
    assert "#define SDM_TRIMAP_MAX_RADIUS 255" in hdr and engine.Engine.TRIMAP_MAX_RADIUS == 255
