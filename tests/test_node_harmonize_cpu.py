"""The CPU side of harmonize: the numpy reference of tests/harmonize_suite.py on its own (its variants, the exact-statistics case, the purpose scenes), the
torch restatement (sdmatte_nodes.harmonize_map / harmonize_cutout) against it, the opt-in node, and the agreement of header, bindings and library.  No GPU,
no emulator."""
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


def _restated(*p):
    from comfyui_sdmatte_amd.sdmatte_nodes import harmonize_cutout
    return harmonize_cutout(*p, return_fg=True, return_map=True)


def test_reference_case_list_covers_what_it_should(pkg):
    """On the reference alone: the shapes, sigmas, stage combinations and special subjects of the list; the fp32 variants stay within 1e-4 of fp64 in
    every output (the largest are the sequential run sums of variant 0 at full strengths), so the tolerance is a tight one."""
    import harmonize_suite as HS
    specs = HS._case_specs()
    assert {s[1] for s in specs} == {1, 37, 70, 130, 260} and {s[0] for s in specs} == {1, 9, 40, 67}
    assert {s[2] for s in specs} == {0.3, 2.0, 6.0, 16.0} and {s[4] for s in specs} == {1, 3} and {s[3] for s in specs} == set(HS.PATTERNS)
    assert (67, 130) in {s[:2] for s in specs} and (40, 260) in {s[:2] for s in specs}
    assert {HS.stages_on(c[4]) for c in HS.cases()} == {("hz_stats", "hz_finalize", "hz_rows", "hz_compose"), ("hz_stats", "hz_finalize", "hz_compose"),
                                                        ("hz_rows", "hz_compose"), ("hz_compose", )}
    assert {s[6] for s in specs} == {None, "tiny", "flat"}
    for name, *_ in HS.cases():
        refs = HS._references(name)
        print(f"[harmonize] {name}: d32 = " + " ".join(f"{d:.3e}" for d in refs[1]))
        assert max(refs[1]) <= 1e-4, name
    # the sub-pixel subject keeps the identity, the flat one has rho at its clamp: g = 1 + contrast s (4 - 1)
    tiny = HS._references(next(c[0] for c in HS.cases() if "tiny" in c[0]))[0][2]
    assert np.array_equal(tiny, np.tile(np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]), (3, 1)))
    flat = HS._references(next(c[0] for c in HS.cases() if "flat" in c[0]))[0][2]
    assert np.allclose(flat[:, :9].reshape(3, 3, 3), np.eye(3) * 2.5, atol=1e-12)      # M = I + 1.5 (P_l + P_p + P_q)


def test_reference_projectors_and_purpose(pkg):
    """The matrices of the header are the projectors of the opponent coordinates and sum to I; reference(fp64) meets both purposes; the exact case
    asserts its own sensitivity (inside exact_case)."""
    import harmonize_suite as HS
    assert np.allclose(HS.P.sum(0), np.eye(3), atol=1e-15)
    rng = np.random.default_rng(0)
    c = rng.uniform(size=(50, 3))
    o = HS.opponent(c)
    for k in range(3):
        assert np.allclose(c @ HS.P[k].T, o[:, k:k + 1] * HS.K[k], atol=1e-14)      # P_k c = o_k(c) k_k
        assert np.allclose(HS.P[k] @ HS.P[k], HS.P[k], atol=1e-15)
    fg, alpha, bg, params = HS.match_scene()
    HS.check_match_purpose(HS.reference(fg, alpha, bg, *params, dtype=np.float32)[1], "reference fp32")
    with pytest.raises(AssertionError):
        HS.check_match_purpose(fg, "the unmatched subject")
    fg, alpha, bg, params = HS.wrap_scene()
    HS.check_wrap_purpose(HS.reference(fg, alpha, bg, *params, dtype=np.float32)[1], "reference fp32")
    with pytest.raises(AssertionError):
        HS.check_wrap_purpose(fg, "no wrap")
    fg, alpha, bg, params, m64, _ = HS.exact_case()
    for v in (0, 1):
        HS.check_exact(HS.reference(fg, alpha, bg, *params, dtype=np.float32, variant=v)[2], f"reference fp32 variant {v}")


def test_restatement_case_list(pkg):
    import harmonize_suite as HS
    HS.check(_restated, lambda t: t)


def test_restatement_exact_and_purpose(pkg):
    import harmonize_suite as HS
    from comfyui_sdmatte_amd.sdmatte_nodes import harmonize_map
    fg, alpha, bg, params, _, _ = HS.exact_case()
    HS.check_exact(harmonize_map(*_t(fg, alpha, bg), *params[:3]).numpy(), "torch restatement")
    fg, alpha, bg, params = HS.match_scene()
    HS.check_match_purpose(_restated(*_t(fg, alpha, bg), *params)[1].numpy(), "torch restatement")
    fg, alpha, bg, params = HS.wrap_scene()
    HS.check_wrap_purpose(_restated(*_t(fg, alpha, bg), *params)[1].numpy(), "torch restatement")


def test_restatement_identities(pkg):
    """What the header states bit for bit holds for the restatement too (identities 1, 2, 3, 5 for a batch, 6)."""
    import harmonize_suite as HS
    fg, alpha, bg = _t(*HS.inputs("dirty", 3, 2, 40, 70))
    a = torch.from_numpy(HS.sanitise_alpha(alpha.numpy()))
    params = (0.6, 0.8, 0.5, 0.5, 2.0)
    out, fgo, m = _restated(fg, alpha, bg, *params)
    assert torch.equal(out[a == 0.0], bg[a == 0.0])
    assert torch.equal(out[a == 1.0], fgo[a == 1.0]) and not torch.equal(out, fgo)
    out0, fgo0, m0 = _restated(fg, alpha, bg, 0.0, 0.0, 0.0, 0.0, 2.0)
    assert torch.equal(fgo0, fg) and torch.equal(out0, a.unsqueeze(-1) * fg + (1.0 - a).unsqueeze(-1) * bg)
    assert torch.equal(m0, torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]).repeat(2, 1))
    for b in range(2):
        assert torch.equal(m[b:b + 1], _restated(fg[b:b + 1], alpha[b:b + 1], bg[b:b + 1], *params)[2]), b
    rep = _restated(fg, alpha, bg[:1].repeat(2, 1, 1, 1), *params)
    assert all(torch.equal(x, y) for x, y in zip(rep, _restated(fg, alpha, bg[:1], *params)))


def test_argument_checks(pkg):
    """ValueError from the restatement (the limits are Engine._check_harmonize_params, which Engine.harmonize uses too)."""
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.sdmatte_nodes import harmonize_cutout, harmonize_map
    assert Engine.HARMONIZE_MAX_WRAP_SIGMA == 16
    fg, a, bg = torch.rand(2, 10, 12, 3), torch.rand(2, 10, 12), torch.rand(1, 10, 12, 3)
    nan, inf = float("nan"), float("inf")
    for k in ("luma_strength", "chroma_strength", "contrast_strength", "wrap_strength"):
        for v in (-0.01, 1.01, nan, inf, "1"):
            with pytest.raises(ValueError):
                harmonize_cutout(fg, a, bg, **{k: v})
    for v in (0.0, -2.0, 16.5, nan, inf):
        with pytest.raises(ValueError):
            harmonize_cutout(fg, a, bg, wrap_sigma=v)
    assert harmonize_cutout(fg, a, bg, wrap_strength=0.0, wrap_sigma=nan).shape == fg.shape      # without the wrap the sigma is not looked at
    with pytest.raises(ValueError):
        harmonize_map(fg, a, bg, luma_strength=2.0)
    for bad in ((fg[..., :2], a, bg), (fg, a[:1], bg), (fg[0], a[0], bg[0]), (fg, a, bg[:, :5]), (fg, a, torch.rand(3, 10, 12, 3))):
        with pytest.raises(ValueError):
            harmonize_cutout(*bad)
    for kw in ({"luma_strength": 1.0}, {"chroma_strength": 0.0}, {"contrast_strength": 1.0}, {"wrap_strength": 1.0}, {"wrap_sigma": 16.0}, {"wrap_sigma": 0.05}):
        assert harmonize_cutout(fg, a, bg, **kw).shape == fg.shape


def test_node_mappings_and_harmonize_node(pkg):
    """Every argument combination of node_mappings returns what it returned (its argument list is unchanged); with_harmonize_node adds exactly
    SDMatteHarmonize and leaves its argument alone."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    from comfyui_sdmatte_amd.engine import Engine
    assert list(inspect.signature(N.node_mappings).parameters)[-2:] == ["motion", "defocus"]
    for flags in itertools.product((False, True), repeat=11):
        base = N.node_mappings(*flags)
        assert "SDMatteHarmonize" not in base[0]
        assert N.with_harmonize_node(base, False) == base
        classes, names = N.with_harmonize_node(base, True)
        assert classes == dict(base[0], SDMatteHarmonize=N.SDMatteHarmonize) and names == dict(base[1], SDMatteHarmonize="SDMatte Harmonize")
        assert "SDMatteHarmonize" not in base[0] and N.with_harmonize_node(base) == (classes, names)
    f = N.SDMatteHarmonize
    it = f.INPUT_TYPES()
    assert f.RETURN_TYPES == ("IMAGE", "IMAGE") and f.RETURN_NAMES == ("image", "foreground") and f.CATEGORY == "Matting/SDMatte"
    assert list(inspect.signature(getattr(f, f.FUNCTION)).parameters) == ["self"] + list(it["required"]) + list(it["optional"])
    assert it["required"]["foreground"][0] == "IMAGE" and it["required"]["alpha"][0] == "MASK" and it["required"]["background"][0] == "IMAGE"
    assert it["optional"]["wrap_sigma"][1]["max"] == Engine.HARMONIZE_MAX_WRAP_SIGMA and it["optional"]["force_cpu"][1]["default"] is False
    defaults = {k: v.default for k, v in inspect.signature(Engine.harmonize).parameters.items() if v.default is not inspect.Parameter.empty}
    assert list(defaults) == ["luma_strength", "chroma_strength", "contrast_strength", "wrap_strength", "wrap_sigma", "return_fg", "return_map", "sync"]
    rdefaults = {k: v.default for k, v in inspect.signature(N.harmonize_cutout).parameters.items() if v.default is not inspect.Parameter.empty}
    for k, spec in it["optional"].items():
        assert spec[1]["tooltip"], k
        if k in Engine.HARMONIZE_DEFAULTS:
            assert spec[1]["default"] == defaults[k] == rdefaults[k] == Engine.HARMONIZE_DEFAULTS[k], k
            if k != "wrap_sigma":
                assert spec[1]["min"] == 0.0 and spec[1]["max"] == 1.0, k


def test_node_cpu_path_and_background_fitting(pkg):
    """force_cpu=True is the restatement, argument by argument; a 2-D mask is one image; one background serves a batch; a background of another size is
    scaled to cover the frame and centre-cropped."""
    import harmonize_suite as HS
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    fg, alpha, bg = _t(*HS.inputs("soft", 2, 2, 24, 40))
    node = N.SDMatteHarmonize()
    out, fgo = node.harmonize(fg, alpha, bg, 0.5, 0.7, 0.3, 0.4, 2.0, force_cpu=True)
    want = N.harmonize_cutout(fg, alpha, bg, 0.5, 0.7, 0.3, 0.4, 2.0, return_fg=True)
    assert torch.equal(out, want[0]) and torch.equal(fgo, want[1]) and out.shape == fg.shape
    out, _ = node.harmonize(fg, alpha, bg[:1], force_cpu=True)
    assert torch.equal(out, N.harmonize_cutout(fg, alpha, bg[:1]))
    out, _ = node.harmonize(fg[:1], alpha[0], bg[:1], wrap_sigma=1.0, force_cpu=True)
    assert torch.equal(out, N.harmonize_cutout(fg[:1], alpha[:1], bg[:1], wrap_sigma=1.0)) and out.shape == (1, 24, 40, 3)
    # fitting: the right size passes through; a wider one keeps its height and loses its sides; a constant one stays constant; the result covers the frame
    assert torch.equal(N.fit_background(bg, 24, 40), bg)
    wide = torch.rand(1, 24, 80, 3)
    assert torch.equal(N.fit_background(wide, 24, 40), wide[:, :, 20:60])
    big = torch.zeros(1, 48, 120, 3)
    big[:, :, 60:] = 1.0                                     # left half black, right half white: scaled by 1 / 2, cropped to the middle 40 of 60 columns
    fit = N.fit_background(big, 24, 40)
    assert fit.shape == (1, 24, 40, 3) and float(fit[:, :, :19].abs().max()) <= 1e-6 and float((fit[:, :, 21:] - 1.0).abs().max()) <= 1e-6
    const = N.fit_background(torch.full((1, 7, 5, 3), 0.25), 24, 40)
    assert const.shape == (1, 24, 40, 3) and float((const - 0.25).abs().max()) <= 1e-6
    out, _ = node.harmonize(fg, alpha, big, force_cpu=True)
    assert torch.equal(out, N.harmonize_cutout(fg, alpha, fit))
    for bad in ((fg[..., :2], alpha, bg), (fg, alpha[:, :5], bg), (fg, alpha, bg[..., :2]), (fg, alpha, torch.rand(3, 24, 40, 3))):
        with pytest.raises(ValueError):      # input validation comes before any engine is looked for
            node.harmonize(*bad)


def test_harmonize_node_env_opt_in(pkg):
    """The module-level mappings follow SDMATTE_HARMONIZE_NODE, independently of the other flags: a fresh interpreter each."""
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; p = load_package(); "
            "print(sorted(p.NODE_CLASS_MAPPINGS), sorted(p.NODE_DISPLAY_NAME_MAPPINGS))" % ROOT)
    flags = ("SDMATTE_EXTRA_NODES", "SDMATTE_FOREGROUND_NODE", "SDMATTE_REFINE_NODE", "SDMATTE_CLEAN_NODE", "SDMATTE_ROI_NODE", "SDMATTE_CANVAS_NODE",
             "SDMATTE_SUBJECTS_NODE", "SDMATTE_EDGE_NODES", "SDMATTE_VIDEO_NODE", "SDMATTE_MOTION_NODE", "SDMATTE_DEFOCUS_NODE", "SDMATTE_HARMONIZE_NODE")
    for defocus, harmonize, want in ((None, None, "['SDMatteApply']"), (None, "0", "['SDMatteApply']"), ("1", None, "['SDMatteApply', 'SDMatteDefocus']"),
                                     (None, "1", "['SDMatteApply', 'SDMatteHarmonize']"), ("1", "1", "['SDMatteApply', 'SDMatteDefocus', 'SDMatteHarmonize']")):
        env = {k: v for k, v in os.environ.items() if k not in flags}
        env.update({k: v for k, v in (("SDMATTE_DEFOCUS_NODE", defocus), ("SDMATTE_HARMONIZE_NODE", harmonize)) if v is not None})
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.strip() == f"{want} {want}", (defocus, harmonize, r.stdout, r.stderr)


def test_product_library_exports_harmonize_call(pkg):
    """The gfx950 library exports the product call, and header, bindings and kernels agree on the limits, the defaults and the launches."""
    from comfyui_sdmatte_amd import build, engine
    dll = ctypes.CDLL(build.build_all())
    assert "sdm_harmonize" in engine.EXPORTS
    getattr(dll, "sdm_harmonize")
    hdr = open(os.path.join(ROOT, "include", "sdmatte.h")).read()
    E = engine.Engine
    d = E.HARMONIZE_DEFAULTS
    for line in (f"#define SDM_HZ_MAX_WRAP_SIGMA {E.HARMONIZE_MAX_WRAP_SIGMA}\n", f"#define SDM_HZ_LUMA_STRENGTH {d['luma_strength']}f\n",
                 f"#define SDM_HZ_CHROMA_STRENGTH {d['chroma_strength']}f\n", f"#define SDM_HZ_CONTRAST_STRENGTH {d['contrast_strength']}f\n",
                 f"#define SDM_HZ_WRAP_STRENGTH {d['wrap_strength']}f\n", f"#define SDM_HZ_WRAP_SIGMA {d['wrap_sigma']}f\n", "#define SDM_HZ_RUN 4096\n",
                 f"#define SDM_HZ_VAR_FLOOR {2.0 ** -20!r}\n", "#define SDM_HZ_MAX_GAIN 4\n", "#define SDM_HZ_MIN_WEIGHT 1.0\n"):
        assert line in hdr, line
    src = open(os.path.join(ROOT, "comfyui-sdmatte_amd", "csrc", "sdm_engine.cpp")).read()
    for k in ("hz_stats", "hz_finalize", "hz_rows", "hz_compose"):
        assert src.count(f'count_kernel("{k}")') == 1 and f"`{k}`" in hdr, k
    kern = open(os.path.join(ROOT, "comfyui-sdmatte_amd", "csrc", "k_harmonize.h")).read()
    assert "#define SDM_HZ_R 48 " in kern and "#define SDM_HZ_RUN_PX 4096 " in kern
