"""The CPU side of the background defocus: the numpy reference of tests/defocus_suite.py on its own (the two variants, the purpose scenes), the torch
restatement (sdmatte_nodes.defocus_background) against it, the opt-in node, and the agreement of header, bindings and library.  No GPU, no emulator."""
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


def _t(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)) for a in arrays)


def test_reference_variants_agree_and_fp32_distance(pkg):
    """Per case, on the reference alone: the two variants agree in fp64 (asserted inside references_for), and the two fp32 evaluations stay within 1e-4
    of fp64, so the tolerance of `compare` is a tight one.  The half widths are those of the closed disc."""
    import defocus_suite as DS
    assert len(DS.cases()) >= 14
    assert sorted({c[5][0] for c in DS.cases()}) == [1, 2, 5, 17, 32, 64]
    for name, *_ in DS.cases():
        refs = DS._references(name)
        print(f"[defocus] {name}: d32 = {refs[1]:.3e} tol = {DS.tolerance(refs[1]):.3e}")
        assert refs[1] <= 1e-4, name
    for R in (1, 2, 5, 17, 32, 64):
        hw = DS.half_widths(R)
        assert all(h * h + dy * dy <= R * R < (h + 1) * (h + 1) + dy * dy for dy, h in enumerate(hw))
        assert DS.disc_size(R) == sum(2 * hw[abs(dy)] + 1 for dy in range(-R, R + 1))


def test_reference_meets_the_purpose_and_the_naive_blur_does_not(pkg):
    import defocus_suite as DS
    image, alpha = DS.purpose_scene()
    ref = lambda im, a, fg, bg, *p: torch.from_numpy(DS.reference(im.numpy(), a.numpy(), fg, bg, *p, dtype=np.float32))
    DS.check_purpose(ref(*_t(image, alpha), None, None, DS.PURPOSE_R, 0.0, 0.5).numpy(), "reference fp32")
    DS.check_disc_shape(ref, lambda t: t, "reference fp32")
    naive = DS.naive_blur_then_lerp(image, alpha, DS.PURPOSE_R)
    with pytest.raises(AssertionError):
        DS.check_purpose(naive, "naive blur")


def test_restatement_case_list(pkg):
    import defocus_suite as DS
    from comfyui_sdmatte_amd.sdmatte_nodes import defocus_background
    DS.check(defocus_background, lambda t: t)


def test_restatement_purpose_and_disc_shape(pkg):
    import defocus_suite as DS
    from comfyui_sdmatte_amd.sdmatte_nodes import defocus_background
    image, alpha = _t(*DS.purpose_scene())
    DS.check_purpose(defocus_background(image, alpha, None, None, DS.PURPOSE_R, 0.0, 0.5).numpy(), "torch restatement")
    DS.check_disc_shape(defocus_background, lambda t: t, "torch restatement")


def test_restatement_identities(pkg):
    """What the header states bit for bit holds for the restatement too: a == 1 gives F, a zero channel gives a F, a batch equals its images."""
    import defocus_suite as DS
    from comfyui_sdmatte_amd.sdmatte_nodes import defocus_background as defocus
    image, alpha, fg, bg = _t(*DS.inputs("dirty", 3, 2, 40, 70, planes=True))
    a = torch.from_numpy(DS.sanitise_alpha(alpha.numpy()))
    out = defocus(image, alpha, fg, bg, 5, 4.0, 0.5)
    assert torch.equal(out[a == 1.0], fg[a == 1.0]) and not torch.equal(out, fg)
    assert torch.equal(defocus(image, alpha, None, None, 5)[a == 1.0], image[a == 1.0])
    bg0 = bg.clone(); bg0[..., 1] = 0.0
    assert torch.equal(defocus(image, alpha, fg, bg0, 5, 4.0, 0.5)[..., 1], a * fg[..., 1])
    for b in range(2):
        assert torch.equal(out[b:b + 1], defocus(image[b:b + 1], alpha[b:b + 1], fg[b:b + 1], bg[b:b + 1], 5, 4.0, 0.5)), b


def test_argument_checks(pkg):
    """ValueError from the restatement (the limits are Engine._check_defocus_params, which Engine.defocus_background uses too)."""
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.sdmatte_nodes import defocus_background as defocus
    assert Engine.DEFOCUS_MAX_RADIUS == 64 and Engine.DEFOCUS_MAX_GAIN == 64
    img, a = torch.rand(2, 10, 12, 3), torch.rand(2, 10, 12)
    nan, inf = float("nan"), float("inf")
    for kw in ({"radius_px": 0}, {"radius_px": 65}, {"radius_px": 1.5}, {"radius_px": "4"}, {"highlight_gain": -0.01}, {"highlight_gain": 64.5},
               {"highlight_gain": nan}, {"highlight_gain": inf}, {"highlight_threshold": -0.1}, {"highlight_threshold": 1.01}, {"highlight_threshold": nan}):
        with pytest.raises(ValueError):
            defocus(img, a, **kw)
    for bad in ((img[..., :2], a), (img, a[:1]), (img[0], a[0])):
        with pytest.raises(ValueError):
            defocus(*bad)
    with pytest.raises(ValueError):
        defocus(img, a, fg=img[:1])
    with pytest.raises(ValueError):
        defocus(img, a, bg=img[:, :5])
    for kw in ({"radius_px": 1}, {"radius_px": 64}, {"highlight_gain": 64.0}, {"highlight_threshold": 0.0}, {"highlight_threshold": 1.0}):
        assert defocus(img, a, **kw).shape == img.shape


def test_node_mappings_with_defocus(pkg):
    """Every earlier argument combination returns what it returned; defocus=True adds exactly SDMatteDefocus."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    from comfyui_sdmatte_amd.engine import Engine
    for flags in itertools.product((False, True), repeat=10):
        base_c, base_n = N.node_mappings(*flags)
        assert N.node_mappings(*flags, False) == (base_c, base_n) == N.node_mappings(*flags, defocus=False)
        assert "SDMatteDefocus" not in base_c
        classes, names = N.node_mappings(*flags, defocus=True)
        assert classes == dict(base_c, SDMatteDefocus=N.SDMatteDefocus) == N.node_mappings(*flags, True)[0]
        assert names == dict(base_n, SDMatteDefocus="SDMatte Defocus Background")
    assert list(inspect.signature(N.node_mappings).parameters)[-2:] == ["motion", "defocus"]
    assert N.node_mappings(False) == ({"SDMatteApply": N.SDMatteApply}, {"SDMatteApply": "Apply SDMatte"})
    f = N.SDMatteDefocus
    it = f.INPUT_TYPES()
    assert f.RETURN_TYPES == ("IMAGE", ) and f.CATEGORY == "Matting/SDMatte"
    assert list(inspect.signature(getattr(f, f.FUNCTION)).parameters) == ["self"] + list(it["required"]) + list(it["optional"])
    assert it["required"]["image"][0] == "IMAGE" and it["required"]["alpha"][0] == "MASK"
    assert it["optional"]["foreground"][0] == "IMAGE" and it["optional"]["background"][0] == "IMAGE"
    assert it["optional"]["radius_px"][1]["max"] == Engine.DEFOCUS_MAX_RADIUS and it["optional"]["radius_px"][1]["min"] == 1
    assert it["optional"]["highlight_gain"][1]["max"] == Engine.DEFOCUS_MAX_GAIN
    assert it["optional"]["force_cpu"][1]["default"] is False and it["optional"]["decontaminate"][1]["default"] is False
    defaults = {k: v.default for k, v in inspect.signature(Engine.defocus_background).parameters.items() if v.default is not inspect.Parameter.empty}
    assert list(defaults) == ["fg", "bg", "radius_px", "highlight_gain", "highlight_threshold", "sync"]
    for k, spec in it["optional"].items():
        assert spec[1]["tooltip"], k
        if k in Engine.DEFOCUS_DEFAULTS:
            assert spec[1]["default"] == defaults[k] == Engine.DEFOCUS_DEFAULTS[k], k


def test_node_cpu_path_equals_restatement(pkg):
    """force_cpu=True is the restatement, argument by argument; a 2-D mask is one image; decontaminate is estimate_foreground, then the call."""
    import defocus_suite as DS
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    image, alpha, fg, bg = _t(*DS.inputs("soft", 2, 2, 24, 40, planes=True))
    node = N.SDMatteDefocus()
    out, = node.defocus(image, alpha, fg, bg, 5, 4.0, 0.5, force_cpu=True)
    assert torch.equal(out, N.defocus_background(image, alpha, fg, bg, 5, 4.0, 0.5)) and out.shape == image.shape
    out, = node.defocus(image, alpha, force_cpu=True)
    assert torch.equal(out, N.defocus_background(image, alpha))
    out, = node.defocus(image[:1], alpha[0], radius_px=3, force_cpu=True)
    assert torch.equal(out, N.defocus_background(image[:1], alpha[:1], radius_px=3)) and out.shape == (1, 24, 40, 3)
    # decontaminate: with neither plane connected, both planes of estimate_foreground (its defaults) feed the call ...
    efg, ebg, _ = N.estimate_foreground(image, alpha)
    out, = node.defocus(image, alpha, radius_px=4, decontaminate=True, force_cpu=True)
    assert torch.equal(out, N.defocus_background(image, alpha, efg, ebg, 4)) and not torch.equal(out, N.defocus_background(image, alpha, None, None, 4))
    # ... and with a plane connected the switch changes nothing
    out, = node.defocus(image, alpha, background=bg, radius_px=4, decontaminate=True, force_cpu=True)
    assert torch.equal(out, N.defocus_background(image, alpha, None, bg, 4))
    for bad in ((image[..., :2], alpha), (image, alpha[:, :5]), (image, alpha, fg[:1]), (image, alpha, None, bg[:, :3])):
        with pytest.raises(ValueError):      # input validation comes before any engine is looked for
            node.defocus(*bad)


def test_defocus_node_env_opt_in(pkg):
    """The module-level mappings follow SDMATTE_DEFOCUS_NODE, independently of the other flags: a fresh interpreter each."""
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; p = load_package(); "
            "print(sorted(p.NODE_CLASS_MAPPINGS), sorted(p.NODE_DISPLAY_NAME_MAPPINGS))" % ROOT)
    flags = ("SDMATTE_EXTRA_NODES", "SDMATTE_FOREGROUND_NODE", "SDMATTE_REFINE_NODE", "SDMATTE_CLEAN_NODE", "SDMATTE_ROI_NODE", "SDMATTE_CANVAS_NODE",
             "SDMATTE_SUBJECTS_NODE", "SDMATTE_EDGE_NODES", "SDMATTE_VIDEO_NODE", "SDMATTE_MOTION_NODE", "SDMATTE_DEFOCUS_NODE")
    for motion, defocus, want in ((None, None, "['SDMatteApply']"), (None, "0", "['SDMatteApply']"), ("1", None, "['SDMatteApply', 'SDMatteTemporalSmoothMotion']"),
                                  (None, "1", "['SDMatteApply', 'SDMatteDefocus']"),
                                  ("1", "1", "['SDMatteApply', 'SDMatteDefocus', 'SDMatteTemporalSmoothMotion']")):
        env = {k: v for k, v in os.environ.items() if k not in flags}
        env.update({k: v for k, v in (("SDMATTE_MOTION_NODE", motion), ("SDMATTE_DEFOCUS_NODE", defocus)) if v is not None})
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.strip() == f"{want} {want}", (motion, defocus, r.stdout, r.stderr)


def test_product_library_exports_defocus_call(pkg):
    """The gfx950 library exports the product call, and header, bindings and kernels agree on the limits, the defaults and the two launches."""
    from comfyui_sdmatte_amd import build, engine
    dll = ctypes.CDLL(build.build_all())
    assert "sdm_defocus_background" in engine.EXPORTS
    getattr(dll, "sdm_defocus_background")
    hdr = open(os.path.join(ROOT, "include", "sdmatte.h")).read()
    E = engine.Engine
    for line in (f"#define SDM_DEFOCUS_MAX_RADIUS {E.DEFOCUS_MAX_RADIUS}\n", f"#define SDM_DEFOCUS_MAX_GAIN {E.DEFOCUS_MAX_GAIN}\n",
                 f"#define SDM_DEFOCUS_RADIUS {E.DEFOCUS_DEFAULTS['radius_px']}\n", f"#define SDM_DEFOCUS_HIGHLIGHT_GAIN {E.DEFOCUS_DEFAULTS['highlight_gain']}f\n",
                 f"#define SDM_DEFOCUS_HIGHLIGHT_THRESHOLD {E.DEFOCUS_DEFAULTS['highlight_threshold']}f\n", f"#define SDM_DEFOCUS_FLOOR {2.0 ** -10}f\n"):
        assert line in hdr, line
    assert "`dof_prefix` then `dof_gather`" in hdr
    src = open(os.path.join(ROOT, "comfyui-sdmatte_amd", "csrc", "sdm_engine.cpp")).read()
    assert src.count('count_kernel("dof_prefix")') == 1 and src.count('count_kernel("dof_gather")') == 1
    kern = open(os.path.join(ROOT, "comfyui-sdmatte_amd", "csrc", "k_defocus.h")).read()
    assert f"#define SDM_DOF_R {E.DEFOCUS_MAX_RADIUS} " in kern
