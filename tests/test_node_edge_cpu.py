"""The CPU side of the distance-field calls: the restatements of sdmatte_nodes against the brute force and the closed forms of tests/edge_suite.py, the
two opt-in nodes, and the agreement of header, bindings and library.  No GPU and no emulator."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def test_distance_field_restatement_equals_brute_force(pkg):
    import edge_suite as ES
    from comfyui_sdmatte_amd.sdmatte_nodes import distance_field
    for name, plane, thr, want in ES.field_cases("brute"):
        got = distance_field(torch.from_numpy(plane), thr)
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want), name


def test_distance_field_restatement_equals_closed_forms(pkg):
    import edge_suite as ES
    from comfyui_sdmatte_amd.sdmatte_nodes import distance_field
    plane, field = ES.seed_case(100, 180, 12)
    assert np.array_equal(distance_field(torch.from_numpy(plane)).numpy(), field)
    assert np.array_equal(distance_field(torch.from_numpy(1.0 - plane)).numpy(), -field)
    plane, field = ES.long_row_case(4096, 1000)
    assert np.array_equal(distance_field(torch.from_numpy(plane)).numpy(), field)
    assert int(distance_field(torch.zeros(1, 3, 4))[0, 0, 0]) == -ES.NONE and int(distance_field(torch.ones(1, 3, 4))[0, 2, 3]) == ES.NONE


def test_field_restatement_gives_the_trimap(pkg):
    """The field's relation to sdm_make_trimap, on the CPU restatements of both."""
    import edge_suite as ES
    import trimap_suite as TS
    from comfyui_sdmatte_amd.sdmatte_nodes import distance_field, trimap_from_mask
    mask = torch.from_numpy(TS.blobs(9, 2, 97, 131))
    field = distance_field(mask, 0.5).numpy()
    for e, d in ((0, 0), (1, 2), (10, 10), (40, 3)):
        assert np.array_equal(trimap_from_mask(mask, 0.5, e, d).numpy(), ES.trimap_from_field(field, e, d)), (e, d)


def test_offset_mask_restatement_consequences(pkg):
    """The three exact consequences of the header, in fp32 on the CPU, for r in {0, 1, 7, 255, 1024}; fp64 exists and agrees to rounding."""
    import edge_suite as ES
    from comfyui_sdmatte_amd.sdmatte_nodes import offset_mask
    mask, field = ES.wide_case()
    fg = field > 0
    d2 = np.where(fg, 0, -field)
    m = torch.from_numpy(mask)
    for r in (0, 1, 7, 255, 1024):
        got = offset_mask(m, float(r), 1.0).numpy()
        assert got.dtype == np.float32
        assert np.array_equal(got == 1.0, d2 <= r * r) and np.array_equal(got > 0.0, d2 < (r + 1) * (r + 1)), r
    assert np.array_equal(offset_mask(m, 0.0, 1.0).numpy(), fg.astype(np.float32))
    r64 = offset_mask(m, 40.0, 12.5, dtype=torch.float64)
    assert r64.dtype == torch.float64 and float((offset_mask(m, 40.0, 12.5).double() - r64).abs().max()) < 1e-4
    # shrinking: -3 leaves 1.0 only where the nearest pixel outside F is at least 3.5 + 0.5 away; the 3 x 4 clump has no such pixel
    assert float(offset_mask(m, -3.0, 1.0).max()) == 0.0
    for bad in (dict(offset_px=2000.0), dict(feather_px=0.5), dict(threshold=1.0), dict(offset_px=float("nan"))):
        with pytest.raises(ValueError):
            offset_mask(m, **bad)


def test_outline_restatement_properties(pkg):
    import edge_suite as ES
    from comfyui_sdmatte_amd.sdmatte_nodes import distance_field, outline_cutout

    class CpuEngine:      # the restatement behind the engine's signature, for the shared property check
        @staticmethod
        def outline(fg, alpha, *args, **kw):
            return outline_cutout(fg, alpha, *args, **kw)
    ES.check_outline_exact_properties(CpuEngine, lambda t: t)
    fg, alpha = ES.outline_inputs(45, 70, 1)
    rgb, A = outline_cutout(fg, alpha, 4.0, (1.0, 0.0, 0.0), "outside")
    assert rgb.dtype == torch.float32 and A.dtype == torch.float32 and rgb.shape == fg.shape and A.shape == alpha.shape
    ring = (A == 1.0) & (torch.nan_to_num(alpha, nan=0.0) == 0.0)
    assert bool(ring.any()) and bool((rgb[ring] == torch.tensor([1.0, 0.0, 0.0])).all())      # no subject: exactly the stroke's colour
    assert outline_cutout(fg, alpha, 4.0, dtype=torch.float64)[0].dtype == torch.float64
    # inside / centre strokes do not change the silhouette's outside
    far = torch.from_numpy(ES.trimap_from_field(distance_field(alpha, 0.5).numpy(), 0, 3) == 0.0)
    a_clean = torch.nan_to_num(alpha, nan=0.0).clamp(0.0, 1.0)
    assert torch.equal(outline_cutout(fg, alpha, 4.0, position="inside")[1][far], a_clean[far])
    for bad in (dict(width_px=0.0), dict(position="around"), dict(opacity=2.0), dict(softness_px=0.0), dict(color=(1.0, 2.0)), dict(edge_threshold=1.0)):
        with pytest.raises(ValueError):
            outline_cutout(fg, alpha, **bad)


def test_node_mappings_with_edge(pkg):
    """Every earlier argument combination returns what it returned; edge=True adds exactly the two distance-field nodes."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    from comfyui_sdmatte_amd.engine import Engine
    assert N.node_mappings(False) == ({"SDMatteApply": N.SDMatteApply}, {"SDMatteApply": "Apply SDMatte"})
    for flags in ((False, ) * 7, (True, False, True, False, True, False, True), (True, ) * 7):
        base_c, base_n = N.node_mappings(*flags)
        assert N.node_mappings(*flags, False) == (base_c, base_n) == N.node_mappings(*flags, edge=False)
        assert "SDMatteOffsetMask" not in base_c and "SDMatteOutline" not in base_c
        classes, names = N.node_mappings(*flags, edge=True)
        assert classes == dict(base_c, SDMatteOffsetMask=N.SDMatteOffsetMask, SDMatteOutline=N.SDMatteOutline)
        assert names == dict(base_n, SDMatteOffsetMask="SDMatte Grow / Shrink Mask", SDMatteOutline="SDMatte Outline")
    for f, rets in ((N.SDMatteOffsetMask, ("MASK", )), (N.SDMatteOutline, ("IMAGE", "MASK"))):
        it = f.INPUT_TYPES()
        assert f.RETURN_TYPES == rets and f.CATEGORY == "Matting/SDMatte"
        assert list(inspect.signature(getattr(f, f.FUNCTION)).parameters) == ["self"] + list(it["required"]) + list(it["optional"])
    it = N.SDMatteOffsetMask.INPUT_TYPES()
    assert it["required"]["mask"][0] == "MASK" and it["required"]["offset_px"][1]["max"] == Engine.DF_MAX_OFFSET == -it["required"]["offset_px"][1]["min"]
    assert it["required"]["feather_px"][1]["max"] == Engine.DF_MAX_FEATHER and it["required"]["feather_px"][1]["min"] == 1.0
    it = N.SDMatteOutline.INPUT_TYPES()
    assert it["required"]["foreground"][0] == "IMAGE" and it["required"]["alpha"][0] == "MASK" and it["required"]["width_px"][1]["max"] == Engine.OUTLINE_MAX_WIDTH
    assert it["required"]["position"][0] == list(Engine.OUTLINE_POSITION) == list(N.OUTLINE_POSITION)
    # the nodes' defaults are the engine calls'
    for f, call in ((N.SDMatteOffsetMask, Engine.offset_mask), (N.SDMatteOutline, Engine.outline)):
        defaults = {k: v.default for k, v in inspect.signature(call).parameters.items() if v.default is not inspect.Parameter.empty}
        inputs = dict(f.INPUT_TYPES()["required"], **f.INPUT_TYPES()["optional"])
        for k in ("offset_px", "feather_px", "threshold", "width_px", "position", "softness_px", "opacity", "edge_threshold"):
            if k in inputs:
                assert inputs[k][1]["default"] == defaults[k], (f.__name__, k)


def test_edge_nodes_cpu_path_equals_restatement(pkg):
    """force_cpu=True is the restatement, argument by argument; a 2-D mask is one image."""
    import edge_suite as ES
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    fg, alpha = ES.outline_inputs(45, 70)
    out, = N.SDMatteOffsetMask().offset(alpha, 3.5, 2.0, 0.3, force_cpu=True)
    assert torch.equal(out, N.offset_mask(alpha, 3.5, 2.0, 0.3)) and out.shape == alpha.shape
    out, = N.SDMatteOffsetMask().offset(alpha[1], -2.0, 1.0, force_cpu=True)
    assert torch.equal(out, N.offset_mask(alpha[1:2], -2.0, 1.0)) and out.shape == (1, 45, 70)
    rgb, A = N.SDMatteOutline().outline(fg, alpha, 5.5, "center", 0.2, 0.4, 0.6, 0.9, 2.0, 0.3, force_cpu=True)
    want = N.outline_cutout(fg, alpha, 5.5, (0.2, 0.4, 0.6), "center", 2.0, 0.9, 0.3)
    assert torch.equal(rgb, want[0]) and torch.equal(A, want[1])
    # input validation comes before any engine is looked for
    for bad in ((fg[..., :2], alpha, 4.0, "outside"), (fg, alpha[:, :5], 4.0, "outside")):
        with pytest.raises(ValueError):
            N.SDMatteOutline().outline(*bad)


def test_edge_nodes_env_opt_in(pkg):
    """The module-level mappings follow SDMATTE_EDGE_NODES, independently of the other flags: a fresh interpreter each."""
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; p = load_package(); "
            "print(sorted(p.NODE_CLASS_MAPPINGS), sorted(p.NODE_DISPLAY_NAME_MAPPINGS))" % ROOT)
    flags = ("SDMATTE_EXTRA_NODES", "SDMATTE_FOREGROUND_NODE", "SDMATTE_REFINE_NODE", "SDMATTE_CLEAN_NODE", "SDMATTE_ROI_NODE", "SDMATTE_CANVAS_NODE",
             "SDMATTE_SUBJECTS_NODE", "SDMATTE_EDGE_NODES")
    for canvas, edge, want in ((None, None, "['SDMatteApply']"), (None, "0", "['SDMatteApply']"),
                               (None, "1", "['SDMatteApply', 'SDMatteOffsetMask', 'SDMatteOutline']"),
                               ("1", "1", "['SDMatteApply', 'SDMatteCanvas', 'SDMatteOffsetMask', 'SDMatteOutline']"), ("1", None, "['SDMatteApply', 'SDMatteCanvas']")):
        env = {k: v for k, v in os.environ.items() if k not in flags}
        env.update({k: v for k, v in (("SDMATTE_CANVAS_NODE", canvas), ("SDMATTE_EDGE_NODES", edge)) if v is not None})
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.strip() == f"{want} {want}", (canvas, edge, r.stdout, r.stderr)


def test_product_library_exports_edge_calls(pkg):
    """The gfx950 library exports the three product calls, and header, bindings and kernels agree on the limits."""
    from comfyui_sdmatte_amd import build, engine, sdmatte_nodes
    dll = ctypes.CDLL(build.build_all())
    for name in ("sdm_distance_field", "sdm_offset_mask", "sdm_outline"):
        assert name in engine.EXPORTS
        getattr(dll, name)
    hdr = open(os.path.join(ROOT, "include", "sdmatte.h")).read()
    E = engine.Engine
    for line in (f"#define SDM_DF_NONE {E.DF_NONE}\n", f"#define SDM_DF_MAX_OFFSET {E.DF_MAX_OFFSET}\n", f"#define SDM_DF_MAX_FEATHER {E.DF_MAX_FEATHER}\n",
                 f"#define SDM_OUTLINE_MAX_WIDTH {E.OUTLINE_MAX_WIDTH}\n"):
        assert line in hdr, line
    assert E.DF_NONE == sdmatte_nodes.DF_NONE == 2 ** 31 - 1 and 2 * 32767 ** 2 < E.DF_NONE
    # the cap's reason: sqrtf(r^2 + 1) > r up to 2048, not at 4096
    for r, holds in ((1024, True), (2048, True), (4096, False)):
        assert (np.sqrt(np.float32(r * r + 1)) > np.float32(r)) == holds, r
    for k in ("df_bits", "df_carry", "df_cols", "df_rows", "df_offset", "df_outline"):
        assert k in hdr, k
