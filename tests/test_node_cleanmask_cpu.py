"""CPU-only checks of the mask clean-up's host side: the restatement `sdmatte_nodes.clean_mask` against the run-based reference of
tests/cleanmask_suite.py on the whole case list, the reference itself against scipy.ndimage.label and by hand, the opt-in node surface and the
exported call."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def test_case_list_covers_the_issue(pkg):
    import cleanmask_suite as CS
    cases = CS.cases()
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    assert {(c[1].shape[1], c[1].shape[2]) for c in cases} == {(1, 1), (1, 300), (300, 1), (CS.T + 1, CS.T - 1), (2 * CS.T + 2, CS.T + 6), (257, 515)}
    assert {n.split("_")[0] for n in names} >= {"empty", "full", "nan", "corners", "checkerboard", "rings", "spiral", "serpentine", "comb", "staircase", "batch",
                                                 "tie", "blobs"}
    assert len({n.split("_")[0] for n, m, *_ in cases if m.shape[0] == 3}) >= 3
    params = {c[2] for c in cases}
    assert set(CS.PARAMS) | {CS.BOTH} <= params
    assert {p[0] for p in params} == {0.0, 0.5, CS.ONE} and {p[4] for p in params} == {False, True}
    stage = {(p[1] > 1 or p[2], p[3] > 0) for p in params}
    assert stage == {(False, False), (True, False), (False, True), (True, True)}
    # something happens: islands go, holes fill, and the oversized min_area empties the mask
    assert min(sum(int(c[4][:, k].sum()) > 0 for c in cases) for k in (1, 2)) >= 2 * len(CS.SHAPES)
    for name, mask, p, want, stats in cases:
        if p[1] == 1 << 28:
            with np.errstate(invalid="ignore"):
                assert not (want > np.float32(p[0])).any(), name


def test_reference_by_hand(pkg):
    import cleanmask_suite as CS
    # checkerboard: one 8-connected component; every inner background pixel is a hole of area 1
    for H, W in ((7, 9), (CS.T + 1, CS.T - 1)):
        cb = CS._checkerboard(1, H, W)
        inner = int((cb[0, 1:-1, 1:-1] == 0).sum())
        out, stats = CS.reference(cb, 0.5, 0, False, 1, False)
        assert stats.tolist() == [[1, 0, inner, inner]] and (out[0, 1:-1, 1:-1] == 1).all() and np.array_equal(out[0, 0], cb[0, 0])
        out, stats = CS.reference(cb, 0.5, 0, False, 0, False)
        assert stats.tolist() == [[1, 0, 0, 0]] and np.array_equal(out, cb)
    # a removed island inside a hole enlarges the hole: ring of 5x5 with a pixel in its middle
    m = np.zeros((1, 9, 9), np.float32)
    m[0, 2:7, 2:7] = 1.0
    m[0, 3:6, 3:6] = 0.0
    m[0, 4, 4] = 1.0
    out, stats = CS.reference(m, 0.5, 2, False, 8, False)           # hole of 8 pixels + the removed pixel = 9 > 8: stays open
    assert stats.tolist() == [[2, 1, 0, 1]] and out[0, 4, 4] == 0.0 and out[0, 3, 3] == 0.0
    out, stats = CS.reference(m, 0.5, 2, False, 9, False)
    assert stats.tolist() == [[2, 1, 1, 10]] and (out[0, 2:7, 2:7] == 1.0).all()
    out, stats = CS.reference(m, 0.5, 0, False, 8, False)           # without stage A the island stays and the hole (8 pixels) fills around it
    assert stats.tolist() == [[2, 0, 1, 8]] and (out[0, 2:7, 2:7] == 1.0).all()
    # a diagonal is one 8-connected component, six 4-connected ones, and cuts the 4-connected background in two
    d = np.eye(6, dtype=bool)
    assert len(CS.components(d, True)) == 1 and len(CS.components(d, False)) == 6 and len(CS.components(~d, False)) == 2 and len(CS.components(~d, True)) == 1
    # tie: the first component in pixel order wins
    t = CS._tie(1, 20, 50)
    out, stats = CS.reference(t, 0.5, 0, True, 0, False)
    assert stats[0, 0] == 3 and stats[0, 1] == 2 and (out[0, 0, 40:] == 1).all() and out[0, 19].sum() == 0
    # batch pair: images are independent
    bp = CS._batch_pair(3, 5, 8)
    out, stats = CS.reference(bp, 0.5, 2, False, 0, False)
    assert stats[:, 0].tolist() == [5, 5, 5] and stats[:, 1].tolist() == [4, 4, 4]


def test_reference_equals_scipy_label(pkg):
    """The run-based components against scipy.ndimage.label: ones((3, 3)) for the foreground, the default cross for the background."""
    ndi = pytest.importorskip("scipy.ndimage")
    import cleanmask_suite as CS
    seen = 0
    for name, mask, p, _, _ in CS.cases():
        if p != CS.BOTH:
            continue
        with np.errstate(invalid="ignore"):
            fg = mask[0] > np.float32(0.5)
        for cls, diagonal, structure in ((fg, True, np.ones((3, 3), int)), (~fg, False, None)):
            lab, n = ndi.label(cls, structure=structure)
            comps = CS.components(cls, diagonal)
            assert len(comps) == n, name
            ours = np.zeros(cls.shape, np.int64)
            for i, c in enumerate(comps):
                for y, x0, x1 in c:
                    ours[y, x0:x1] = i + 1
            # the same partition: the pairs (our id, scipy's id) are a bijection
            pairs = np.unique(np.stack([ours.ravel(), lab.ravel()]), axis=1)
            assert pairs.shape[1] == n + (1 if (~cls).any() else 0), name
        seen += 1
    assert seen == len(CS.SHAPES) * len(CS.PATTERNS)


def test_clean_mask_restatement_equals_reference(pkg):
    import cleanmask_suite as CS
    from comfyui_sdmatte_amd.sdmatte_nodes import clean_mask
    CS.check_clean_mask(lambda m, *p: clean_mask(m, *p, return_stats=True), lambda t: t)
    m = torch.from_numpy(CS.blobs(1, 2, 40, 50))
    assert CS.same_bits(clean_mask(m, 0.5, 6, False, 5).numpy(), CS.reference(m.numpy(), 0.5, 6, False, 5)[0])      # without return_stats: one tensor


def test_clean_mask_argument_checks(pkg):
    from comfyui_sdmatte_amd.sdmatte_nodes import clean_mask
    m = torch.rand(1, 6, 7)
    for bad in ({"threshold": 1.0}, {"threshold": -0.1}, {"threshold": float("nan")}, {"threshold": float("inf")}, {"threshold": 1.0 - 1e-9},
                {"min_area": -1}, {"min_area": (1 << 28) + 1}, {"min_area": 2.5}, {"max_hole_area": -1}, {"max_hole_area": (1 << 28) + 1}):
        with pytest.raises(ValueError):
            clean_mask(m, **bad)
    with pytest.raises(ValueError):
        clean_mask(m[0])
    with pytest.raises(ValueError):
        clean_mask(torch.zeros(1, 0, 4))
    out, stats = clean_mask(m, 0.0, 1 << 28, True, 1 << 28, True, return_stats=True)
    assert out.shape == m.shape and out.dtype == torch.float32 and stats.shape == (1, 4) and stats.dtype == torch.int32


def test_node_mappings_with_clean(pkg):
    """Every earlier argument combination returns what it returned; clean=True adds exactly SDMatteCleanMask."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    classes, names = N.node_mappings(False)
    assert classes == {"SDMatteApply": N.SDMatteApply} and names == {"SDMatteApply": "Apply SDMatte"}
    old = {"SDMatteApply": "Apply SDMatte", "SDMatteTrimapFromMask": "SDMatte Trimap From Mask", "SDMatteApplyMask": "Apply SDMatte (Mask)",
           "SDMatteForeground": "SDMatte Foreground Colours", "SDMatteRefineAlpha": "SDMatte Refine Alpha"}
    for extra in (False, True):
        for fg in (False, True):
            for ref in (False, True):
                base_c, base_n = N.node_mappings(extra, fg, ref)
                want = ["SDMatteApply"] + (["SDMatteTrimapFromMask", "SDMatteApplyMask"] if extra else []) + (["SDMatteForeground"] if fg else []) + (
                    ["SDMatteRefineAlpha"] if ref else [])
                assert list(base_c) == want and base_n == {k: old[k] for k in want}
                assert all(base_c[k] is getattr(N, k) for k in want)
                assert N.node_mappings(extra, fg, ref, False) == (base_c, base_n) == N.node_mappings(extra, foreground=fg, refine=ref, clean=False)
                classes, names = N.node_mappings(extra, fg, ref, clean=True)
                assert classes == dict(base_c, SDMatteCleanMask=N.SDMatteCleanMask)
                assert names == dict(base_n, SDMatteCleanMask="SDMatte Clean Mask")
    f = N.SDMatteCleanMask
    it = f.INPUT_TYPES()
    assert list(it) == ["required"] and list(it["required"]) == ["mask", "threshold", "min_area", "keep_largest", "max_hole_area", "binarize"]
    req = it["required"]
    assert req["mask"][0] == "MASK" and req["threshold"][0] == "FLOAT" and req["threshold"][1]["default"] == 0.5 and req["threshold"][1]["max"] < 1.0
    for k in ("min_area", "max_hole_area"):
        assert req[k][0] == "INT" and (req[k][1]["default"], req[k][1]["min"], req[k][1]["max"]) == (64, 0, 1 << 28)
    for k in ("keep_largest", "binarize"):
        assert req[k][0] == "BOOLEAN" and req[k][1]["default"] is False
    assert f.RETURN_TYPES == ("MASK", ) and f.CATEGORY == "Matting/SDMatte" and callable(getattr(f, f.FUNCTION))
    import inspect
    assert list(inspect.signature(getattr(f, f.FUNCTION)).parameters) == ["self"] + list(req)
    # input validation comes before any engine is looked for
    for bad in ((torch.zeros(1, 2, 8, 8), ), (torch.zeros(0, 8, 8), ), (torch.zeros(1, 8, 8), 1.0), (torch.zeros(1, 8, 8), -0.5), (torch.zeros(1, 8, 8), 0.5, -1),
                (torch.zeros(1, 8, 8), 0.5, 1.5), (torch.zeros(1, 8, 8), 0.5, 3, False, (1 << 28) + 1)):
        with pytest.raises(ValueError):
            f().clean(*bad)


def test_clean_node_env_opt_in(pkg):
    """The module-level mappings follow SDMATTE_CLEAN_NODE, independently of the other flags: a fresh interpreter each."""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; p = load_package(); "
            "print(sorted(p.NODE_CLASS_MAPPINGS), sorted(p.NODE_DISPLAY_NAME_MAPPINGS))" % ROOT)
    flags = ("SDMATTE_EXTRA_NODES", "SDMATTE_FOREGROUND_NODE", "SDMATTE_REFINE_NODE", "SDMATTE_CLEAN_NODE")
    for extra, clean, want in ((None, None, "['SDMatteApply']"), (None, "0", "['SDMatteApply']"), (None, "1", "['SDMatteApply', 'SDMatteCleanMask']"),
                               ("1", "1", "['SDMatteApply', 'SDMatteApplyMask', 'SDMatteCleanMask', 'SDMatteTrimapFromMask']")):
        env = {k: v for k, v in os.environ.items() if k not in flags}
        env.update({k: v for k, v in (("SDMATTE_EXTRA_NODES", extra), ("SDMATTE_CLEAN_NODE", clean)) if v is not None})
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.strip() == f"{want} {want}", (extra, clean, r.stdout, r.stderr)


def test_product_library_exports_clean_mask(pkg):
    """The gfx950 library exports the new product call, and header and bindings agree on the limits."""
    from comfyui_sdmatte_amd import build, engine
    dll = ctypes.CDLL(build.build_all())
    assert "sdm_clean_mask" in engine.EXPORTS
    getattr(dll, "sdm_clean_mask")
    hdr = open(os.path.join(ROOT, "include", "sdmatte.h")).read()
    assert "#define SDM_CLEAN_STATS 4" in hdr and f"#define SDM_FG_MAX_PIXELS {engine.Engine.CLEAN_MAX_AREA} " in hdr
