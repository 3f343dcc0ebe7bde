"""The subject's box on the CPU: sdmatte_nodes.subject_roi against the brute force of tests/roi_suite.py, paste_roi, the opt-in node
SDMatteApplyROI and the mappings.  No GPU, no emulator."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def test_subject_roi_restatement_equals_brute_force(pkg):
    import roi_suite as RS
    from comfyui_sdmatte_amd.sdmatte_nodes import subject_roi
    names = set()
    for name, plane, thr, mpx, mpct, sq in RS.box_cases():
        got = subject_roi(torch.from_numpy(plane), thr, mpx, mpct, sq)
        want = RS.brute_force(plane, thr, mpx, mpct, sq)
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want), (name, got.tolist(), want.tolist())
        y0, x0, h, w = (got[:, k] for k in range(4))
        H, W = plane.shape[1:]
        assert bool(((y0 >= 0) & (x0 >= 0) & (h >= 1) & (w >= 1) & (y0 + h <= H) & (x0 + w <= W)).all()), name
        names.add(name)
    assert len(names) == len(RS.box_cases())


def test_subject_roi_cases_mean_what_their_names_say(pkg):
    """The case list really holds the situations it names: clipping on each side, a product that integer division truncates, the three square cases."""
    import roi_suite as RS
    cases = {c[0]: c for c in RS.box_cases()}

    def box(name):
        _, plane, thr, mpx, mpct, sq = cases[name]
        return RS.brute_force(plane, thr, mpx, mpct, sq)[0].tolist()
    H, W = 97, 131
    assert box("empty") == [0, 0, H, W] == box("empty_at_threshold") == box("whole_frame")
    assert box("single_pixel_top_left") == [0, 0, 1, 1] and box("single_pixel_bottom_right") == [H - 1, W - 1, 1, 1]
    assert box("single_pixel_centre") == [H // 2, W // 2, 1, 1]
    assert box("nan_is_outside") == [38, 48, 24, 44]
    assert box("margin_clips_top")[0] == 0 and box("margin_clips_left")[1] == 0
    b = box("margin_clips_bottom")
    assert b[0] + b[2] == H and b[0] == 60
    b = box("margin_clips_right")
    assert b[1] + b[3] == W and b[1] == 80
    assert box("margin_pct_not_divisible") == [20 - 3, 30 - 1, 37 + 6, 13 + 2]              # 1 + 259 // 100 = 3, 1 + 91 // 100 = 1
    assert box("margin_pct_33") == [20 - 3, 30 - 9, 11 + 6, 29 + 18]
    assert box("square_hits_top") == [0, 29, 72, 72] and box("square_hits_left") == [9, 0, 72, 72]
    assert box("square_hits_bottom") == [H - 72, 29, 72, 72] and box("square_hits_right") == [9, W - 72, 72, 72]
    assert box("square_frame_shorter_than_L") == [0, 38, 20, 104] and box("square_frame_narrower_than_L") == [38, 0, 104, 20]
    assert box("square_odd_growth") == [40 - 12, 30, 30, 30]
    assert cases["soft_threshold_0.3_96x128"][2] == 0.3 and box("soft_threshold_0.3_96x128") != box("vector_path_96x128")


def test_subject_roi_argument_checks(pkg):
    from comfyui_sdmatte_amd.sdmatte_nodes import subject_roi
    p = torch.rand(1, 6, 7)
    for bad in ({"roi_threshold": 1.0}, {"roi_threshold": -0.1}, {"roi_threshold": float("nan")}, {"roi_threshold": float("inf")},
                {"roi_threshold": 1.0 - 1e-9}, {"margin_px": -1}, {"margin_px": 4097}, {"margin_px": 2.5}, {"margin_pct": -1}, {"margin_pct": 101}):
        with pytest.raises(ValueError):
            subject_roi(p, **bad)
    with pytest.raises(ValueError):
        subject_roi(p[0])
    with pytest.raises(ValueError):
        subject_roi(torch.zeros(1, 0, 4))
    out = subject_roi(p, 0.0, 4096, 100, True)
    assert out.tolist() == [[0, 0, 6, 7]] and out.dtype == torch.int32


def test_paste_roi(pkg):
    from comfyui_sdmatte_amd.sdmatte_nodes import paste_roi
    crop = torch.arange(24, dtype=torch.float32).view(2, 3, 4) + 1.0
    roi = torch.tensor([[1, 2, 3, 4], [4, 0, 3, 4]], dtype=torch.int32)
    out = paste_roi(crop, roi, 7, 6)
    assert out.shape == (2, 7, 6) and out.dtype == torch.float32
    assert torch.equal(out[0, 1:4, 2:6], crop[0]) and torch.equal(out[1, 4:7, 0:4], crop[1])
    assert float(out.sum()) == float(crop.sum())                                           # 0.0 everywhere else
    assert torch.equal(paste_roi([crop[0], crop[1]], roi.numpy(), 7, 6), out)              # a list of planes, a numpy box
    for bad in ((crop, roi[:1]), (crop[:, :2], roi), (crop, torch.tensor([[1, 3, 3, 4], [4, 0, 3, 4]])), (crop, torch.tensor([[5, 2, 3, 4], [4, 0, 3, 4]]))):
        with pytest.raises(ValueError):
            paste_roi(bad[0], bad[1], 7, 6)


def test_node_mappings_with_roi(pkg):
    """Every earlier argument combination returns what it returned; roi=True adds exactly SDMatteApplyROI."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    from comfyui_sdmatte_amd.engine import Engine
    old = {"SDMatteApply": "Apply SDMatte", "SDMatteTrimapFromMask": "SDMatte Trimap From Mask", "SDMatteApplyMask": "Apply SDMatte (Mask)",
           "SDMatteForeground": "SDMatte Foreground Colours", "SDMatteRefineAlpha": "SDMatte Refine Alpha", "SDMatteCleanMask": "SDMatte Clean Mask"}
    assert N.node_mappings(False) == ({"SDMatteApply": N.SDMatteApply}, {"SDMatteApply": "Apply SDMatte"})
    for extra in (False, True):
        for fg in (False, True):
            for ref in (False, True):
                for clean in (False, True):
                    base_c, base_n = N.node_mappings(extra, fg, ref, clean)
                    want = ["SDMatteApply"] + (["SDMatteTrimapFromMask", "SDMatteApplyMask"] if extra else []) + (["SDMatteForeground"] if fg else []) + (
                        ["SDMatteRefineAlpha"] if ref else []) + (["SDMatteCleanMask"] if clean else [])
                    assert list(base_c) == want and base_n == {k: old[k] for k in want}
                    assert all(base_c[k] is getattr(N, k) for k in want)
                    assert N.node_mappings(extra, fg, ref, clean, False) == (base_c, base_n) == N.node_mappings(extra, foreground=fg, refine=ref, clean=clean, roi=False)
                    classes, names = N.node_mappings(extra, fg, ref, clean, roi=True)
                    assert classes == dict(base_c, SDMatteApplyROI=N.SDMatteApplyROI)
                    assert names == dict(base_n, SDMatteApplyROI="Apply SDMatte (Subject Box)")
    f = N.SDMatteApplyROI
    it = f.INPUT_TYPES()
    mask_req = N.SDMatteApplyMask.INPUT_TYPES()["required"]
    box = ["roi_threshold", "margin_px", "margin_pct", "square"]
    assert [k for k in it["required"] if k not in box] == list(mask_req) and all(it["required"][k] == mask_req[k] for k in mask_req)
    assert [k for k in it["required"] if k in box] == box and it["optional"] == N.SDMatteApplyMask.INPUT_TYPES()["optional"]
    # the node's defaults are the engine call's
    defaults = {k: v.default for k, v in inspect.signature(Engine.apply_matte_roi).parameters.items() if v.default is not inspect.Parameter.empty}
    for k in box + ["threshold", "erode_px", "dilate_px"]:
        assert it["required"][k][1]["default"] == defaults[k], k
    assert {k: v.default for k, v in inspect.signature(Engine.subject_roi).parameters.items() if k in box} == {k: defaults[k] for k in box}
    assert {k: v.default for k, v in inspect.signature(N.subject_roi).parameters.items() if k in box} == {k: defaults[k] for k in box}
    req = it["required"]
    assert req["roi_threshold"][0] == "FLOAT" and req["roi_threshold"][1]["min"] == 0.0 and req["roi_threshold"][1]["max"] < 1.0
    assert (req["margin_px"][0], req["margin_px"][1]["min"], req["margin_px"][1]["max"]) == ("INT", 0, Engine.ROI_MAX_MARGIN_PX)
    assert (req["margin_pct"][0], req["margin_pct"][1]["min"], req["margin_pct"][1]["max"]) == ("INT", 0, 100)
    assert req["square"][0] == "BOOLEAN"
    assert f.RETURN_TYPES == ("MASK", "IMAGE", "MASK", "BBOX") and len(f.RETURN_NAMES) == 4 and f.CATEGORY == "Matting/SDMatte"
    assert list(inspect.signature(getattr(f, f.FUNCTION)).parameters) == ["self"] + list(req) + list(it["optional"])
    # input validation comes before any model is looked for
    img, msk = torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8)
    tail = (64, False, "alpha_only", True, 0.8)
    for bad in ((img[..., :2], msk, 0.5, 1, 1, 0.0, 1, 1, True), (img, msk[:, :4], 0.5, 1, 1, 0.0, 1, 1, True), (img, msk, 0.5, 1, 1, 1.0, 1, 1, True),
                (img, msk, 0.5, 1, 1, 0.0, 4097, 1, True), (img, msk, 0.5, 1, 1, 0.0, 1, 101, True)):
        with pytest.raises(ValueError):
            f().apply_matte("SDMatte.safetensors", *bad, *tail)
    with pytest.raises(RuntimeError):
        f().apply_matte("SDMatte.safetensors", img, msk, 0.5, 1, 1, 0.0, 1, 1, True, *tail, force_cpu=True)


def test_roi_node_env_opt_in(pkg):
    """The module-level mappings follow SDMATTE_ROI_NODE, independently of the other flags: a fresh interpreter each."""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; p = load_package(); "
            "print(sorted(p.NODE_CLASS_MAPPINGS), sorted(p.NODE_DISPLAY_NAME_MAPPINGS))" % ROOT)
    flags = ("SDMATTE_EXTRA_NODES", "SDMATTE_FOREGROUND_NODE", "SDMATTE_REFINE_NODE", "SDMATTE_CLEAN_NODE", "SDMATTE_ROI_NODE")
    for extra, roi, want in ((None, None, "['SDMatteApply']"), (None, "0", "['SDMatteApply']"), (None, "1", "['SDMatteApply', 'SDMatteApplyROI']"),
                             ("1", "1", "['SDMatteApply', 'SDMatteApplyMask', 'SDMatteApplyROI', 'SDMatteTrimapFromMask']")):
        env = {k: v for k, v in os.environ.items() if k not in flags}
        env.update({k: v for k, v in (("SDMATTE_EXTRA_NODES", extra), ("SDMATTE_ROI_NODE", roi)) if v is not None})
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.strip() == f"{want} {want}", (extra, roi, r.stdout, r.stderr)


def test_product_library_exports_roi_calls(pkg):
    """The gfx950 library exports the two new product calls, and header and bindings agree on the limit."""
    from comfyui_sdmatte_amd import build, engine
    dll = ctypes.CDLL(build.build_all())
    for name in ("sdm_subject_roi", "sdm_apply_matte_roi"):
        assert name in engine.EXPORTS
        getattr(dll, name)
    hdr = open(os.path.join(ROOT, "include", "sdmatte.h")).read()
    assert f"#define SDM_ROI_MAX_MARGIN_PX {engine.Engine.ROI_MAX_MARGIN_PX}\n" in hdr
