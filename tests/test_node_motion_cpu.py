"""The CPU side of the motion-compensated temporal smoothing: the numpy reference of tests/motion_suite.py on its own (undecided share, translation,
purpose), the torch restatement (sdmatte_nodes.temporal_smooth_alpha_motion) against it, the opt-in node, and the agreement of header, bindings and
library.  No GPU, no emulator."""
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
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in arrays)


def test_reference_undecided_share_and_fp32_distance(pkg):
    """Per case, on the reference alone: at most 0.5 % of the pixels are undecided, and on the others the two fp32 evaluations stay within 1e-5 of fp64
    (2.3e-7 was the largest on the prototype), so the tolerance of `compare` is a tight one."""
    import motion_suite as MS
    assert len(MS.cases()) >= 24
    for name, *_ in MS.cases():
        refs = MS._references(name)
        print(f"[motion] {name}: undecided {MS.undecided_share(refs) * 100:.3f} % d32 = {refs[2]:.3e}")
        assert MS.undecided_share(refs) <= MS.MAX_UNDECIDED_SHARE, name
        assert refs[2] <= 1e-5, name


def test_reference_search_0_is_the_existing_filter(pkg):
    import motion_suite as MS
    import temporal_suite as TS
    image, alpha = MS.inputs("dirty", 3, 4, 20, 40)
    out, und = MS.reference(image, alpha, 2, 1, 0, 0.1, 0.5, 1.0, 1.0, 0)
    assert np.array_equal(out, TS.reference(image, alpha, 2, 1, 0.1, 1.0, 1.0, 0)) and not und.any()


def test_reference_meets_the_purpose_and_the_existing_filter_does_not(pkg):
    """The fp64 reference meets the four conditions with room (0.426 x for 0.55, 0.748 x for 0.85, 0.107 for 0.230, 0.852 x for 0.95); the existing
    filter leaves the band's flicker above 0.8 x the observed alpha's (0.87 x): that is what the new call adds."""
    import motion_suite as MS
    image, _, obs = MS.purpose_scene()
    MS.check_purpose(MS.reference(image, obs, *MS.PURPOSE)[0], "reference fp64")
    ratio = MS.band_flicker(MS.purpose_existing()) / MS.band_flicker(obs)
    print(f"[motion] existing filter: band flicker {ratio:.3f} x the observed")
    assert ratio > 0.8
    with pytest.raises(AssertionError):
        MS.check_purpose(MS.purpose_existing(), "existing filter")


def test_restatement_case_list(pkg):
    import motion_suite as MS
    from comfyui_sdmatte_amd.sdmatte_nodes import temporal_smooth_alpha_motion
    MS.check(temporal_smooth_alpha_motion, lambda t: t)


def test_restatement_translation_and_purpose(pkg):
    import motion_suite as MS
    from comfyui_sdmatte_amd.sdmatte_nodes import temporal_smooth_alpha_motion
    MS.check_translation(temporal_smooth_alpha_motion, lambda t: t, "torch restatement")
    image, _, obs = MS.purpose_scene()
    MS.check_purpose(temporal_smooth_alpha_motion(*_t(image, obs), *MS.PURPOSE).numpy(), "torch restatement")


def test_restatement_identities(pkg):
    """What the header states bit for bit holds for the restatement too: search 0, the no-op conditions, clips = separate calls, a hard cut = its shots."""
    import motion_suite as MS
    from comfyui_sdmatte_amd.sdmatte_nodes import temporal_smooth_alpha, temporal_smooth_alpha_motion as smooth
    image, alpha = _t(*MS.inputs("dirty", 5, 5, 20, 38))
    a = torch.from_numpy(MS.sanitise_alpha(alpha.numpy()))
    assert not torch.equal(smooth(image, alpha, search=2), a)
    assert torch.equal(smooth(image, alpha, search=0, motion_penalty=0.7), temporal_smooth_alpha(image, alpha))
    assert torch.equal(smooth(image, alpha, search=2, strength=0.0), a)
    assert torch.equal(smooth(image, alpha, search=2, max_change=0.0), a)
    assert torch.equal(smooth(image, alpha, search=2, clip_len=1), a)
    assert torch.equal(smooth(image[:1], alpha[:1], 4, 2, 3), a[:1])
    far = (0.125 * torch.arange(5).float().view(5, 1, 1, 1) + 0.02 * torch.rand(5, 20, 38, 3)).contiguous()      # every D of every candidate >= tau2
    assert torch.equal(smooth(far, alpha, 4, 2, 3, 0.1), a)
    out = smooth(image, alpha, 2, 1, 2, clip_len=2)
    for lo in range(0, 5, 2):
        assert torch.equal(out[lo:lo + 2], smooth(image[lo:lo + 2], alpha[lo:lo + 2], 2, 1, 2)), lo
    image, alpha = _t(*MS.cut_scene(11, 3, 2, 20, 38))
    out = smooth(image, alpha, 4, 1, 3)
    assert torch.equal(out[:3], smooth(image[:3], alpha[:3], 4, 1, 3)) and torch.equal(out[3:], smooth(image[3:], alpha[3:], 4, 1, 3))
    assert float((smooth(image, alpha, search=2, max_change=0.05) - alpha).abs().max()) <= 0.05 + 1e-7


def test_argument_checks(pkg):
    """ValueError from the restatement (the limits are Engine._check_tsm_params, which Engine.smooth_alpha_motion uses too)."""
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.sdmatte_nodes import temporal_smooth_alpha_motion as smooth
    assert Engine.TSM_MAX_SEARCH == 8
    img, a = torch.rand(3, 10, 12, 3), torch.rand(3, 10, 12)
    nan, inf = float("nan"), float("inf")
    for kw in ({"search": -1}, {"search": 9}, {"search": 1.5}, {"search": "4"}, {"motion_penalty": -0.01}, {"motion_penalty": 1.01}, {"motion_penalty": nan},
               {"motion_penalty": inf}, {"radius": 0}, {"radius": 5}, {"patch": -1}, {"patch": 3}, {"clip_len": -1}, {"clip_len": 4},
               {"color_tolerance": 0.0009}, {"color_tolerance": 1.5}, {"color_tolerance": nan}, {"strength": -0.1}, {"strength": 1.1}, {"max_change": -0.1},
               {"max_change": 2.0}, {"max_change": inf}):
        with pytest.raises(ValueError):
            smooth(img, a, **kw)
    for bad in ((img[..., :2], a), (img, a[:2]), (img[0], a[0])):
        with pytest.raises(ValueError):
            smooth(*bad)
    for kw in ({"search": 0}, {"search": 8}, {"motion_penalty": 0.0}, {"motion_penalty": 1.0}, {"search": 0, "motion_penalty": 7.0}):      # (not looked at)
        assert smooth(img, a, **kw).shape == a.shape
    assert smooth(img, a, 4, 2, 8, 1.0 / 1024.0, 1.0, 1.0, 1.0, 3).shape == a.shape


def test_node_mappings_with_motion(pkg):
    """Every earlier argument combination returns what it returned; motion=True adds exactly SDMatteTemporalSmoothMotion."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    from comfyui_sdmatte_amd.engine import Engine
    for flags in itertools.product((False, True), repeat=9):
        base_c, base_n = N.node_mappings(*flags)
        assert N.node_mappings(*flags, False) == (base_c, base_n) == N.node_mappings(*flags, motion=False)
        assert "SDMatteTemporalSmoothMotion" not in base_c
        classes, names = N.node_mappings(*flags, motion=True)
        assert classes == dict(base_c, SDMatteTemporalSmoothMotion=N.SDMatteTemporalSmoothMotion)
        assert names == dict(base_n, SDMatteTemporalSmoothMotion="SDMatte Temporal Smooth (Motion)")
    f = N.SDMatteTemporalSmoothMotion
    it = f.INPUT_TYPES()
    assert f.RETURN_TYPES == ("MASK", ) and f.CATEGORY == "Matting/SDMatte"
    assert list(inspect.signature(getattr(f, f.FUNCTION)).parameters) == ["self"] + list(it["required"]) + list(it["optional"])
    assert it["required"]["image"][0] == "IMAGE" and it["required"]["alpha"][0] == "MASK"
    assert it["optional"]["radius"][1]["max"] == Engine.TS_MAX_RADIUS and it["optional"]["patch"][1]["max"] == Engine.TS_MAX_PATCH
    assert it["optional"]["search"][1]["max"] == Engine.TSM_MAX_SEARCH and it["optional"]["search"][1]["min"] == 0
    assert it["optional"]["force_cpu"][1]["default"] is False
    defaults = {k: v.default for k, v in inspect.signature(Engine.smooth_alpha_motion).parameters.items() if v.default is not inspect.Parameter.empty}
    assert list(defaults) == ["radius", "patch", "search", "color_tolerance", "motion_penalty", "strength", "max_change", "clip_len", "sync"]
    for k, spec in it["optional"].items():
        assert spec[1]["tooltip"], k
        if k != "force_cpu":
            assert spec[1]["default"] == defaults[k] == Engine.TSM_DEFAULTS[k], k


def test_node_cpu_path_equals_restatement(pkg):
    """force_cpu=True is the restatement, argument by argument; a 2-D mask is one frame."""
    import motion_suite as MS
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    image, alpha = _t(*MS.inputs("moving", 2, 4, 20, 30))
    out, = N.SDMatteTemporalSmoothMotion().smooth(image, alpha, 3, 2, 2, 0.05, 0.1, 0.5, 0.2, 3, force_cpu=True)
    assert torch.equal(out, N.temporal_smooth_alpha_motion(image, alpha, 3, 2, 2, 0.05, 0.1, 0.5, 0.2, 3)) and out.shape == alpha.shape
    out, = N.SDMatteTemporalSmoothMotion().smooth(image, alpha, force_cpu=True)
    assert torch.equal(out, N.temporal_smooth_alpha_motion(image, alpha))
    out, = N.SDMatteTemporalSmoothMotion().smooth(image[:1], alpha[0], force_cpu=True)
    assert torch.equal(out, alpha[:1]) and out.shape == (1, 20, 30)
    for bad in ((image[..., :2], alpha), (image, alpha[:, :5])):      # input validation comes before any engine is looked for
        with pytest.raises(ValueError):
            N.SDMatteTemporalSmoothMotion().smooth(*bad)


def test_motion_node_env_opt_in(pkg):
    """The module-level mappings follow SDMATTE_MOTION_NODE, independently of the other flags, and SDMATTE_VIDEO_NODE=1 alone registers what it did: a
    fresh interpreter each."""
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; p = load_package(); "
            "print(sorted(p.NODE_CLASS_MAPPINGS), sorted(p.NODE_DISPLAY_NAME_MAPPINGS))" % ROOT)
    flags = ("SDMATTE_EXTRA_NODES", "SDMATTE_FOREGROUND_NODE", "SDMATTE_REFINE_NODE", "SDMATTE_CLEAN_NODE", "SDMATTE_ROI_NODE", "SDMATTE_CANVAS_NODE",
             "SDMATTE_SUBJECTS_NODE", "SDMATTE_EDGE_NODES", "SDMATTE_VIDEO_NODE", "SDMATTE_MOTION_NODE")
    for video, motion, want in ((None, None, "['SDMatteApply']"), (None, "0", "['SDMatteApply']"), ("1", None, "['SDMatteApply', 'SDMatteTemporalSmooth']"),
                                (None, "1", "['SDMatteApply', 'SDMatteTemporalSmoothMotion']"),
                                ("1", "1", "['SDMatteApply', 'SDMatteTemporalSmooth', 'SDMatteTemporalSmoothMotion']")):
        env = {k: v for k, v in os.environ.items() if k not in flags}
        env.update({k: v for k, v in (("SDMATTE_VIDEO_NODE", video), ("SDMATTE_MOTION_NODE", motion)) if v is not None})
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.strip() == f"{want} {want}", (video, motion, r.stdout, r.stderr)


def test_product_library_exports_motion_call(pkg):
    """The gfx950 library exports the product call, and header, bindings and kernel agree on the limits, the defaults and the one launch."""
    from comfyui_sdmatte_amd import build, engine
    dll = ctypes.CDLL(build.build_all())
    assert "sdm_smooth_alpha_motion" in engine.EXPORTS
    getattr(dll, "sdm_smooth_alpha_motion")
    hdr = open(os.path.join(ROOT, "include", "sdmatte.h")).read()
    E = engine.Engine
    for line in (f"#define SDM_TSM_MAX_SEARCH {E.TSM_MAX_SEARCH}\n", f"#define SDM_TSM_SEARCH {E.TSM_DEFAULTS['search']}\n",
                 f"#define SDM_TSM_MOTION_PENALTY {E.TSM_DEFAULTS['motion_penalty']}f\n"):
        assert line in hdr, line
    assert "tsm_smooth" in hdr
    src = open(os.path.join(ROOT, "comfyui-sdmatte_amd", "csrc", "sdm_engine.cpp")).read()
    assert src.count('count_kernel("tsm_smooth")') == 1 and src.count('count_kernel("ts_smooth")') == 1
    kern = open(os.path.join(ROOT, "comfyui-sdmatte_amd", "csrc", "k_motion.h")).read()
    assert f"#define SDM_TSM_S {E.TSM_MAX_SEARCH} " in kern
