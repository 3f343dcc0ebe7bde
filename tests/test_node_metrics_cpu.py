"""The CPU side of the matte metrics: the two references of tests/metrics_suite.py against each other on every case (the check that the definition was
transcribed right), what each case is for, the torch restatement (sdmatte_nodes.matte_metrics) in fp32 under the suite's rule, the opt-in node, and the
agreement of header, bindings and library.  No GPU, no emulator."""
import ctypes
import inspect
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def test_references_agree_on_every_case(pkg):
    """loop_reference (flood fill, explicit 2-D kernel) and the torch restatement in fp64 (label equivalence, separable filter): the level maps exactly, the
    sums to 1e-12 relative."""
    import metrics_suite as MS
    MS.check_references_agree()


def test_cases_cover_what_they_should(pkg):
    """On the reference alone: the winding component spans the tile seams, the tie and the frozen pixels occur, the empty levels are empty, the exact zeros
    are zeros, the three radii are 1, 4 and 9; every d32 is small, so the tolerance is a tight one."""
    import metrics_suite as MS
    MS.check_case_properties()
    assert {c[1].shape for c in MS.cases()} >= {(2, 70, 133), (1, 65, 130), (1, 15, 12)} and {c[4] for c in MS.cases()} == {0.25, 1.4, 2.0, 4.0}
    assert {c[5] for c in MS.cases()} == {True, False} and any(c[3] is None for c in MS.cases())
    for name, *_ in MS.cases():
        raw64, _, d32, _ = MS.references(name)
        rel = (d32 / np.maximum(1.0, np.abs(raw64)))[:, list(MS.SUM_SLOTS)].max()
        print(f"[metrics] {name}: largest d32 / max(1, |ref|) = {rel:.3e}")
        assert rel <= 1e-5, name
    assert MS.expected_counts(MS.case_calls()) == MS.expected_counts([(c[5], False) for c in MS.cases()]) and all(lv == cn for cn, lv in MS.case_calls())
    assert sum(MS.launches(True).values()) == 63 and sum(MS.launches(False).values()) == 2 and MS.launches(True, True) == MS.launches(True, False)


def test_restatement_fp32_case_list(pkg):
    """The restatement on fp32 tensors is an implementation like any other: exact where the header says so, the sums within the rule."""
    import metrics_suite as MS
    from comfyui_sdmatte_amd.sdmatte_nodes import matte_metrics
    MS.check(lambda pred, gt, tri, sigma, conn, levels: matte_metrics(pred, gt, tri, sigma, conn, return_levels=levels), lambda t: t)


def test_restatement_units_batch_and_argument_checks(pkg):
    from comfyui_sdmatte_amd.sdmatte_nodes import matte_metrics, matte_metric_weights
    import metrics_suite as MS
    pred, gt, tri = (_t(x) for x in MS.batch_of_three())
    res = matte_metrics(pred, gt, tri, return_levels=True)
    raw = res["raw"]
    assert raw.dtype == torch.float64 and raw.shape == (3, 8) and res["levels"].dtype == torch.int32 and res["levels"].shape == pred.shape
    assert torch.equal(res["sad"], raw[:, 1] / 1000) and torch.equal(res["mse"], raw[:, 2] / raw[:, 0]) and torch.equal(res["grad"], raw[:, 3] / 1000)
    assert torch.equal(res["conn"], raw[:, 4] / 1000) and torch.equal(res["n"], raw[:, 0]) and torch.equal(res["max_abs"], raw[:, 5])
    assert torch.equal(res["sad_frame"], raw[:, 6] / 1000) and torch.equal(res["mse_frame"], raw[:, 7] / (70 * 133))
    for b in range(3):
        one = matte_metrics(pred[b:b + 1], gt[b:b + 1], tri[b:b + 1], return_levels=True)
        assert torch.equal(one["raw"], raw[b:b + 1]) and torch.equal(one["levels"], res["levels"][b:b + 1])
    empty = matte_metrics(pred, gt, torch.zeros_like(tri), conn=False)
    assert bool((empty["mse"] == 0).all()) and bool((empty["n"] == 0).all()) and bool((empty["mse_frame"] > 0).all()) and "levels" not in empty
    whole = matte_metrics(pred, gt, None, conn=False)
    assert torch.equal(whole["raw"], matte_metrics(pred, gt, torch.full_like(tri, 0.5), conn=False)["raw"])
    for s, r in ((0.25, 1), (1.4, 4), (4.0, 9)):
        rr, G, D = matte_metric_weights(s)
        wr, wG, wD = MS.weights(s)
        assert rr == r == wr and np.array_equal(G, wG) and np.array_equal(D, wD)
        assert abs(float((np.outer(G.astype(np.float64), D.astype(np.float64)) ** 2).sum()) - 1.0) < 1e-6      # G (x) D has unit L2 norm
    for kw in ({"grad_sigma": 0.2}, {"grad_sigma": 4.5}, {"grad_sigma": float("nan")}, {"conn": False, "return_levels": True}):
        with pytest.raises(ValueError):
            matte_metrics(pred, gt, tri, **kw)
    for args in ((pred, gt[:, :5], tri), (pred, gt, tri[:1]), (pred[0], gt[0], None)):
        with pytest.raises(ValueError):
            matte_metrics(*args)


def test_node_mappings_and_metrics_node(pkg):
    """node_mappings keeps its argument list and its results; with_metrics_node adds exactly SDMatteMetrics and leaves its argument alone."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    from comfyui_sdmatte_amd.engine import Engine
    assert list(inspect.signature(N.node_mappings).parameters)[-2:] == ["motion", "defocus"]
    for flags in itertools.product((False, True), repeat=3):
        base = N.with_harmonize_node(N.node_mappings(flags[0], defocus=flags[1]), flags[2])
        assert "SDMatteMetrics" not in base[0] and N.with_metrics_node(base, False) == base
        classes, names = N.with_metrics_node(base, True)
        assert classes == dict(base[0], SDMatteMetrics=N.SDMatteMetrics) and set(names) == set(classes) and names["SDMatteMetrics"].startswith("SDMatte Metrics")
        assert "SDMatteMetrics" not in base[0] and N.with_metrics_node(base) == (classes, names)
    f = N.SDMatteMetrics
    it = f.INPUT_TYPES()
    assert f.RETURN_TYPES == ("STRING", "FLOAT", "FLOAT", "FLOAT", "FLOAT") and f.RETURN_NAMES == ("report", "sad", "mse", "grad", "conn")
    assert f.CATEGORY == "Matting/SDMatte" and list(inspect.signature(getattr(f, f.FUNCTION)).parameters) == ["self"] + list(it["required"]) + list(it["optional"])
    assert list(it["required"]) == ["alpha", "ground_truth"] and list(it["optional"]) == ["trimap", "grad_sigma", "connectivity", "force_cpu"]
    assert all(it["required"][k][0] == "MASK" for k in it["required"]) and it["optional"]["trimap"][0] == "MASK"
    sig = it["optional"]["grad_sigma"][1]
    assert sig["default"] == Engine.METRICS_GRAD_SIGMA == 1.4 and sig["min"] == 0.25 and sig["max"] == 4.0 and it["optional"]["force_cpu"][1]["default"] is False
    assert all(spec[1]["tooltip"] for spec in list(it["required"].values()) + list(it["optional"].values()))
    defaults = {k: v.default for k, v in inspect.signature(Engine.matte_metrics).parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == {"trimap": None, "grad_sigma": 1.4, "conn": True, "return_levels": False, "sync": True}
    rdefaults = {k: v.default for k, v in inspect.signature(N.matte_metrics).parameters.items() if v.default is not inspect.Parameter.empty}
    assert rdefaults == {"trimap": None, "grad_sigma": 1.4, "conn": True, "return_levels": False}


def test_node_cpu_path_and_report(pkg):
    """force_cpu=True is the restatement; a 2-D mask is one image; the report has a line per image and a mean line; the floats are the batch means."""
    import metrics_suite as MS
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    pred, gt, tri = (_t(x) for x in MS.batch_of_three())
    node = N.SDMatteMetrics()
    text, sad, mse, grad, conn = node.score(pred, gt, tri, force_cpu=True)
    want = N.matte_metrics(pred, gt, tri)
    assert (sad, mse, grad, conn) == tuple(sum(float(v) for v in want[k]) / 3 for k in ("sad", "mse", "grad", "conn"))
    lines = text.split("\n")
    assert len(lines) == 4 and [ln.split(":")[0] for ln in lines] == ["image 0", "image 1", "image 2", "mean"]
    assert all(w in lines[0] for w in ("SAD", "MSE", "Grad", "Conn", "n = ")) and f"{sad:.4f}" in lines[3]
    text, sad, mse, grad, conn = node.score(pred[0], gt[0], grad_sigma=2.0, connectivity=False, force_cpu=True)
    one = N.matte_metrics(pred[:1], gt[:1], None, 2.0, False)
    assert conn == 0.0 and sad == float(one["sad"][0]) and grad == float(one["grad"][0]) and len(text.split("\n")) == 2
    for bad in ((pred, gt[:, :5], None), (pred, gt, tri[:1]), (pred[..., None], gt[..., None], None)):
        with pytest.raises(ValueError):      # input validation comes before any engine is looked for
            node.score(*bad)


def test_metrics_node_env_opt_in(pkg):
    """The module-level mappings follow SDMATTE_METRICS_NODE, independently of the other flags: a fresh interpreter each."""
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; p = load_package(); "
            "print(sorted(p.NODE_CLASS_MAPPINGS), sorted(p.NODE_DISPLAY_NAME_MAPPINGS))" % ROOT)
    flags = ("SDMATTE_EXTRA_NODES", "SDMATTE_FOREGROUND_NODE", "SDMATTE_REFINE_NODE", "SDMATTE_CLEAN_NODE", "SDMATTE_ROI_NODE", "SDMATTE_CANVAS_NODE",
             "SDMATTE_SUBJECTS_NODE", "SDMATTE_EDGE_NODES", "SDMATTE_VIDEO_NODE", "SDMATTE_MOTION_NODE", "SDMATTE_DEFOCUS_NODE", "SDMATTE_HARMONIZE_NODE",
             "SDMATTE_METRICS_NODE")
    for harmonize, metrics, want in ((None, None, "['SDMatteApply']"), (None, "0", "['SDMatteApply']"), (None, "1", "['SDMatteApply', 'SDMatteMetrics']"),
                                     ("1", "1", "['SDMatteApply', 'SDMatteHarmonize', 'SDMatteMetrics']")):
        env = {k: v for k, v in os.environ.items() if k not in flags}
        env.update({k: v for k, v in (("SDMATTE_HARMONIZE_NODE", harmonize), ("SDMATTE_METRICS_NODE", metrics)) if v is not None})
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.strip() == f"{want} {want}", (harmonize, metrics, r.stdout, r.stderr)


def test_product_library_exports_metrics_call(pkg):
    """The gfx950 library exports the product call, and header, bindings and kernels agree on the limits, the defaults and the launches."""
    from comfyui_sdmatte_amd import build, engine
    dll = ctypes.CDLL(build.build_all())
    assert "sdm_matte_metrics" in engine.EXPORTS
    getattr(dll, "sdm_matte_metrics")
    hdr = open(os.path.join(ROOT, "include", "sdmatte.h")).read()
    for line in ("#define SDM_MM_STATS 8\n", f"#define SDM_MM_GRAD_SIGMA {engine.Engine.METRICS_GRAD_SIGMA}f\n", "#define SDM_MM_MAX_GRAD_RADIUS 9\n",
                 "#define SDM_MM_CONN_LEVELS 10\n", "#define SDM_MM_CONN_THETA 0.15f\n"):
        assert line in hdr, line
    assert len(engine.Engine.METRICS_KEYS) == 8
    src = open(os.path.join(ROOT, "comfyui-sdmatte_amd", "csrc", "sdm_engine.cpp")).read()
    for k in ("mm_pixel", "mm_level", "mm_conn", "mm_finalize"):
        assert src.count(f'count_kernel("{k}")') == 1 and f"`{k}`" in hdr, k
    kern = open(os.path.join(ROOT, "comfyui-sdmatte_amd", "csrc", "k_metrics.h")).read()
    for k in ("mm_pixel_kernel", "mm_level_kernel", "mm_conn_kernel", "mm_finalize_kernel"):
        assert f"void {k}(" in kern, k
    assert "atomicAdd" not in kern and '#include "k_metrics.h"' in src
