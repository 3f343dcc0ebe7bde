"""The CPU side of the temporal smoothing: the torch restatement (sdmatte_nodes.temporal_smooth_alpha) against the numpy reference of
tests/temporal_suite.py, the identities of the header on it, the opt-in node, and the agreement of header, bindings and library.  No GPU, no emulator."""
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


def test_reference_meets_the_purpose(pkg):
    """The scene is a fair one: the suite's own reference (fp64) meets the conditions with room (flicker 0.27 x for a bound of 0.5, mean error
    1.007 x for 1.05, max error below the observed alpha's)."""
    import temporal_suite as TS
    image, _, obs = TS.purpose_scene()
    TS.check_purpose(TS.reference(image, obs, *TS.PURPOSE), "reference fp64")


def test_restatement_case_list_and_purpose(pkg):
    import temporal_suite as TS
    from comfyui_sdmatte_amd.sdmatte_nodes import temporal_smooth_alpha
    TS.check(temporal_smooth_alpha, lambda t: t)
    image, _, obs = TS.purpose_scene()
    TS.check_purpose(temporal_smooth_alpha(*_t(image, obs), *TS.PURPOSE).numpy(), "torch restatement")


def test_restatement_identities(pkg):
    """What the header states bit for bit holds for the restatement too: the no-op conditions, clips = separate calls, a hard cut = its two shots."""
    import temporal_suite as TS
    from comfyui_sdmatte_amd.sdmatte_nodes import temporal_smooth_alpha as smooth
    image, alpha = _t(*TS._inputs("dirty", 5, 7, 33, 70))
    a = torch.from_numpy(TS.sanitise_alpha(alpha.numpy()))
    assert not torch.equal(smooth(image, alpha), a)
    assert torch.equal(smooth(image, alpha, strength=0.0), a)
    assert torch.equal(smooth(image, alpha, max_change=0.0), a)
    assert torch.equal(smooth(image, alpha, clip_len=1), a)
    assert torch.equal(smooth(image[:1], alpha[:1], 4, 2), a[:1])
    far = (0.125 * torch.arange(7).float().view(7, 1, 1, 1) + 0.02 * torch.rand(1, 33, 70, 3)).expand(7, 33, 70, 3).contiguous()
    assert torch.equal(smooth(far, alpha, 4, 2, 0.1), a)
    out = smooth(image, alpha, 2, 1, clip_len=3)
    for lo in range(0, 7, 3):
        assert torch.equal(out[lo:lo + 3], smooth(image[lo:lo + 3], alpha[lo:lo + 3], 2, 1)), lo
    image, alpha = _t(*TS.cut_scene(11, 5, 4, 33, 70))
    out = smooth(image, alpha, 4, 2)
    assert torch.equal(out[:5], smooth(image[:5], alpha[:5], 4, 2)) and torch.equal(out[5:], smooth(image[5:], alpha[5:], 4, 2))
    # max_change is a bound on the distance to the frame's own alpha
    assert float((smooth(image, alpha, max_change=0.05) - alpha).abs().max()) <= 0.05 + 1e-7


def test_restatement_argument_checks(pkg):
    from comfyui_sdmatte_amd.sdmatte_nodes import temporal_smooth_alpha as smooth
    img, a = torch.rand(3, 10, 12, 3), torch.rand(3, 10, 12)
    for kw in ({"radius": 0}, {"radius": 5}, {"patch": -1}, {"patch": 3}, {"clip_len": -1}, {"clip_len": 4}, {"color_tolerance": 0.0009},
               {"color_tolerance": 1.5}, {"color_tolerance": float("nan")}, {"strength": -0.1}, {"strength": 1.1}, {"max_change": -0.1}, {"max_change": 2.0},
               {"max_change": float("inf")}):
        with pytest.raises(ValueError):
            smooth(img, a, **kw)
    for bad in ((img[..., :2], a), (img, a[:2]), (img[0], a[0])):
        with pytest.raises(ValueError):
            smooth(*bad)
    assert smooth(img, a, 4, 2, 1.0 / 1024.0, 1.0, 1.0, 3).shape == a.shape


def test_node_mappings_with_video(pkg):
    """Every earlier argument combination returns what it returned; video=True adds exactly SDMatteTemporalSmooth."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    from comfyui_sdmatte_amd.engine import Engine
    assert N.node_mappings(False) == ({"SDMatteApply": N.SDMatteApply}, {"SDMatteApply": "Apply SDMatte"})
    for flags in itertools.product((False, True), repeat=8):
        base_c, base_n = N.node_mappings(*flags)
        assert N.node_mappings(*flags, False) == (base_c, base_n) == N.node_mappings(*flags, video=False)
        assert "SDMatteTemporalSmooth" not in base_c
        classes, names = N.node_mappings(*flags, video=True)
        assert classes == dict(base_c, SDMatteTemporalSmooth=N.SDMatteTemporalSmooth)
        assert names == dict(base_n, SDMatteTemporalSmooth="SDMatte Temporal Smooth")
    f = N.SDMatteTemporalSmooth
    it = f.INPUT_TYPES()
    assert f.RETURN_TYPES == ("MASK", ) and f.CATEGORY == "Matting/SDMatte"
    assert list(inspect.signature(getattr(f, f.FUNCTION)).parameters) == ["self"] + list(it["required"]) + list(it["optional"])
    assert it["required"]["image"][0] == "IMAGE" and it["required"]["alpha"][0] == "MASK"
    assert it["optional"]["radius"][1]["max"] == Engine.TS_MAX_RADIUS and it["optional"]["patch"][1]["max"] == Engine.TS_MAX_PATCH
    assert it["optional"]["force_cpu"][1]["default"] is False
    # the node's defaults are the engine call's, and every input has a tooltip
    defaults = {k: v.default for k, v in inspect.signature(Engine.smooth_alpha_temporal).parameters.items() if v.default is not inspect.Parameter.empty}
    for k, spec in it["optional"].items():
        assert spec[1]["tooltip"], k
        if k != "force_cpu":
            assert spec[1]["default"] == defaults[k] == Engine.TS_DEFAULTS[k], k


def test_node_cpu_path_equals_restatement(pkg):
    """force_cpu=True is the restatement, argument by argument; a 2-D mask is one frame."""
    import temporal_suite as TS
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    image, alpha = _t(*TS._inputs("moving", 2, 6, 20, 30))
    out, = N.SDMatteTemporalSmooth().smooth(image, alpha, 3, 2, 0.05, 0.5, 0.2, 4, force_cpu=True)
    assert torch.equal(out, N.temporal_smooth_alpha(image, alpha, 3, 2, 0.05, 0.5, 0.2, 4)) and out.shape == alpha.shape
    out, = N.SDMatteTemporalSmooth().smooth(image, alpha, force_cpu=True)
    assert torch.equal(out, N.temporal_smooth_alpha(image, alpha))
    out, = N.SDMatteTemporalSmooth().smooth(image[:1], alpha[0], force_cpu=True)
    assert torch.equal(out, alpha[:1]) and out.shape == (1, 20, 30)
    # input validation comes before any engine is looked for
    for bad in ((image[..., :2], alpha), (image, alpha[:, :5])):
        with pytest.raises(ValueError):
            N.SDMatteTemporalSmooth().smooth(*bad)


def test_video_node_env_opt_in(pkg):
    """The module-level mappings follow SDMATTE_VIDEO_NODE, independently of the other flags: a fresh interpreter each."""
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; p = load_package(); "
            "print(sorted(p.NODE_CLASS_MAPPINGS), sorted(p.NODE_DISPLAY_NAME_MAPPINGS))" % ROOT)
    flags = ("SDMATTE_EXTRA_NODES", "SDMATTE_FOREGROUND_NODE", "SDMATTE_REFINE_NODE", "SDMATTE_CLEAN_NODE", "SDMATTE_ROI_NODE", "SDMATTE_CANVAS_NODE",
             "SDMATTE_SUBJECTS_NODE", "SDMATTE_EDGE_NODES", "SDMATTE_VIDEO_NODE")
    for canvas, video, want in ((None, None, "['SDMatteApply']"), (None, "0", "['SDMatteApply']"), (None, "1", "['SDMatteApply', 'SDMatteTemporalSmooth']"),
                                ("1", "1", "['SDMatteApply', 'SDMatteCanvas', 'SDMatteTemporalSmooth']")):
        env = {k: v for k, v in os.environ.items() if k not in flags}
        env.update({k: v for k, v in (("SDMATTE_CANVAS_NODE", canvas), ("SDMATTE_VIDEO_NODE", video)) if v is not None})
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.strip() == f"{want} {want}", (canvas, video, r.stdout, r.stderr)


def test_product_library_exports_temporal_call(pkg):
    """The gfx950 library exports the product call, and header, bindings and kernel agree on the limits and on the one launch."""
    from comfyui_sdmatte_amd import build, engine
    dll = ctypes.CDLL(build.build_all())
    assert "sdm_smooth_alpha_temporal" in engine.EXPORTS
    getattr(dll, "sdm_smooth_alpha_temporal")
    hdr = open(os.path.join(ROOT, "include", "sdmatte.h")).read()
    E = engine.Engine
    for line in (f"#define SDM_TS_MAX_RADIUS {E.TS_MAX_RADIUS}\n", f"#define SDM_TS_MAX_PATCH {E.TS_MAX_PATCH}\n"):
        assert line in hdr, line
    assert "ts_smooth" in hdr and "ONE kernel launch" in hdr
    src = open(os.path.join(ROOT, "comfyui-sdmatte_amd", "csrc", "sdm_engine.cpp")).read()
    assert src.count('count_kernel("ts_smooth")') == 1
