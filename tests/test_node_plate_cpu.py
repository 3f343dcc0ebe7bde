"""The CPU side of the clean plate: the numpy reference of tests/plate_suite.py on its own (fp32 distance, the purpose scene), the torch restatement
(sdmatte_nodes.clean_plate) against it, the opt-in node, and the agreement of header, bindings and library.  No GPU, no emulator."""
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


def _t(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)) for a in arrays)


def _ref32(image, alpha, bg=None, hole=None, alpha_cut=0.0625):
    import plate_suite as PS
    n = lambda t: None if t is None else t.numpy()
    return torch.from_numpy(PS.reference(n(image), n(alpha), n(bg), n(hole), alpha_cut, np.float32))


def test_reference_fp32_distance_and_case_list(pkg):
    """Per case, on the reference alone: fp32 stays within 1e-6 of fp64 (convex combinations only), so the tolerance of `compare` is a tight one; the
    list holds the sizes, the cuts and the optional planes the kernels branch on."""
    import plate_suite as PS
    cases = PS.cases()
    sizes = {c[1].shape[1:3] for c in cases}
    assert {(1, 1), (1, 300), (300, 1), (2, 3), (32, 32), (33, 31), (37, 70), (67, 131), (129, 257), (200, 300)} <= sizes
    assert {c[5] for c in cases} == {1.0, 0.25, 0.0625, 2.0 ** -10} and any(c[1].shape[0] == 3 for c in cases)
    assert {(c[3] is not None, c[4] is not None) for c in cases} == {(False, False), (False, True), (True, False), (True, True)}
    for name, *_ in cases:
        refs = PS._references(name)
        print(f"[plate] {name}: d32 = {refs[1]:.3e} tol = {PS.tolerance(refs[1]):.3e}")
        assert refs[1] <= 1e-6, name
    # the disc of radius 80 is filled from beyond one group of three levels: its centre lies 80 pixels = more than 2^3 * 8 from the nearest background
    name, image, alpha, *_ = next(c for c in cases if "disc80" in c[0])
    assert PS.levels_beyond_small(200, 300) == 4 and alpha[0, 90, 165] == 1.0


def test_reference_meets_the_purpose_and_the_identities(pkg):
    import plate_suite as PS
    PS.check_purpose(_ref32, lambda t: t, "reference fp32")
    r64, d32, ref_err, mean_err = PS.purpose_reference()
    # the numbers of the suite's docstring
    assert abs(ref_err[0] - 0.0675) < 5e-4 and abs(ref_err[1] - 0.0160) < 5e-4 and abs(mean_err[0] - 0.1706) < 5e-4 and abs(mean_err[1] - 0.0606) < 5e-4
    for H, W in PS.IDENTITY_SIZES:
        PS.check_identities(_ref32, lambda t: t, H, W, "reference fp32")
    # a fill that reads the subject through fails the purpose
    image, alpha, _ = PS.purpose_scene()
    with pytest.raises(AssertionError):
        PS.check_purpose(lambda im, a, bg, hole, cut: im if bg is None else bg, lambda t: t, "no fill")


def test_restatement_case_list(pkg):
    import plate_suite as PS
    from comfyui_sdmatte_amd.sdmatte_nodes import clean_plate
    PS.check(clean_plate, lambda t: t)
    # fp64 is the reference in fp64, to rounding
    for name, image, alpha, bg, hole, cut in PS.cases()[:8]:
        out = clean_plate(*_t(image, alpha, bg, hole), cut, dtype=torch.float64)
        assert out.dtype == torch.float64 and float(np.abs(out.numpy() - PS._references(name)[0]).max()) <= 1e-12, name


def test_restatement_purpose_and_identities(pkg):
    """What the header states bit for bit holds for the restatement too."""
    import plate_suite as PS
    from comfyui_sdmatte_amd.sdmatte_nodes import clean_plate
    PS.check_purpose(clean_plate, lambda t: t, "torch restatement")
    for H, W in PS.IDENTITY_SIZES:
        PS.check_identities(clean_plate, lambda t: t, H, W, "torch restatement")
    image, alpha, bg, hole = _t(*PS.inputs("dirty", 3, 2, 40, 70, with_bg=True, with_hole=True))
    out = clean_plate(image, alpha, bg, hole, 0.25)
    for b in range(2):
        assert torch.equal(out[b:b + 1], clean_plate(image[b:b + 1], alpha[b:b + 1], bg[b:b + 1], hole[b:b + 1], 0.25)), b
    alpha[0] = 1.0
    assert bool((clean_plate(image, alpha)[0] == 0.0).all())


def test_argument_checks(pkg):
    """ValueError from the restatement (the limits are those of Engine.fill_background)."""
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.sdmatte_nodes import clean_plate
    assert Engine.PLATE_ALPHA_CUT == 0.0625 and Engine.PLATE_MIN_CUT == 2.0 ** -10
    img, a = torch.rand(2, 10, 12, 3), torch.rand(2, 10, 12)
    nan, inf = float("nan"), float("inf")
    for cut in (0.0, 2.0 ** -11, -1.0, 1.001, nan, inf, "0.5"):
        with pytest.raises(ValueError):
            clean_plate(img, a, alpha_cut=cut)
    for bad in ((img[..., :2], a), (img, a[:1]), (img[0], a[0])):
        with pytest.raises(ValueError):
            clean_plate(*bad)
    with pytest.raises(ValueError):
        clean_plate(img, a, bg=img[:1])
    with pytest.raises(ValueError):
        clean_plate(img, a, hole=a[:, :5])
    with pytest.raises(ValueError):
        clean_plate(img, a, dtype=torch.float16)
    for cut in (2.0 ** -10, 1.0):
        assert clean_plate(img, a, alpha_cut=cut).shape == img.shape
    defaults = {k: v.default for k, v in inspect.signature(Engine.fill_background).parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == {"bg": None, "hole": None, "alpha_cut": Engine.PLATE_ALPHA_CUT, "sync": True}
    assert inspect.signature(clean_plate).parameters["alpha_cut"].default == Engine.PLATE_ALPHA_CUT


def test_with_plate_node(pkg):
    """with_plate_node adds exactly SDMatteCleanPlate and does not modify its argument; the node's inputs match its function."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    from comfyui_sdmatte_amd.engine import Engine
    base = N.with_tiled_node(N.node_mappings(True), True)
    before = (dict(base[0]), dict(base[1]))
    classes, names = N.with_plate_node(base)
    assert base == before and N.with_plate_node(base, False) == before
    assert classes == dict(before[0], SDMatteCleanPlate=N.SDMatteCleanPlate) and names == dict(before[1], SDMatteCleanPlate="SDMatte Clean Plate (Fill Background)")
    f = N.SDMatteCleanPlate
    it = f.INPUT_TYPES()
    assert f.RETURN_TYPES == ("IMAGE", ) and f.CATEGORY == "Matting/SDMatte"
    assert list(inspect.signature(getattr(f, f.FUNCTION)).parameters) == ["self"] + list(it["required"]) + list(it["optional"])
    assert it["required"]["image"][0] == "IMAGE" and it["required"]["alpha"][0] == "MASK"
    assert it["optional"]["hole"][0] == "MASK" and it["optional"]["background"][0] == "IMAGE"
    cut = it["optional"]["alpha_cut"][1]
    assert cut["default"] == Engine.PLATE_ALPHA_CUT and cut["min"] == Engine.PLATE_MIN_CUT and cut["max"] == 1.0
    assert it["optional"]["force_cpu"][1]["default"] is False and it["optional"]["decontaminate"][1]["default"] is False
    assert all(spec[1]["tooltip"] for spec in it["optional"].values())
    assert "SDMATTE_PLATE_NODE=1" in N.__doc__


def test_node_cpu_path_equals_restatement(pkg):
    """force_cpu=True is the restatement, argument by argument; a 2-D mask is one image; decontaminate is estimate_foreground's background plane, then
    the call."""
    import plate_suite as PS
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    image, alpha, bg, hole = _t(*PS.inputs("soft", 2, 2, 24, 40, with_bg=True, with_hole=True))
    node = N.SDMatteCleanPlate()
    out, = node.fill(image, alpha, hole, bg, 0.25, force_cpu=True)
    assert torch.equal(out, N.clean_plate(image, alpha, bg, hole, 0.25)) and out.shape == image.shape
    out, = node.fill(image, alpha, force_cpu=True)
    assert torch.equal(out, N.clean_plate(image, alpha))
    out, = node.fill(image[:1], alpha[0], hole=hole[0], alpha_cut=1.0, force_cpu=True)
    assert torch.equal(out, N.clean_plate(image[:1], alpha[:1], None, hole[:1], 1.0)) and out.shape == (1, 24, 40, 3)
    _, ebg, _ = N.estimate_foreground(image, alpha)
    out, = node.fill(image, alpha, alpha_cut=1.0, decontaminate=True, force_cpu=True)
    assert torch.equal(out, N.clean_plate(image, alpha, ebg, None, 1.0)) and not torch.equal(out, N.clean_plate(image, alpha, None, None, 1.0))
    out, = node.fill(image, alpha, background=bg, alpha_cut=1.0, decontaminate=True, force_cpu=True)      # a connected plane wins
    assert torch.equal(out, N.clean_plate(image, alpha, bg, None, 1.0))
    for bad in ((image[..., :2], alpha), (image, alpha[:, :5]), (image, alpha, hole[:, :3]), (image, alpha, None, bg[:1])):
        with pytest.raises(ValueError):      # input validation comes before any engine is looked for
            node.fill(*bad)


class _StubEngine:
    """Engine.fill_background / estimate_foreground by their restatements, with a record of the calls."""

    def __init__(self):
        self.calls = []

    def estimate_foreground(self, image, alpha, sync=True):
        from comfyui_sdmatte_amd.sdmatte_nodes import estimate_foreground
        self.calls.append(("estimate_foreground", sync))
        fg, bg, _ = estimate_foreground(image, alpha)
        return fg, bg

    def fill_background(self, image, alpha, bg=None, hole=None, alpha_cut=0.0625, sync=True):
        from comfyui_sdmatte_amd.sdmatte_nodes import clean_plate
        self.calls.append(("fill_background", bg is not None, hole is not None, alpha_cut, sync))
        return clean_plate(image, alpha, bg, hole, alpha_cut)


def test_node_engine_path_against_a_stub_engine(pkg, monkeypatch):
    """Without force_cpu the node calls the engine once (twice with decontaminate, the plane handed over without a sync) and returns a CPU image."""
    import plate_suite as PS
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    eng = _StubEngine()
    monkeypatch.setattr(N, "_torch_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(N, "_trimap_engine", lambda device: eng)
    image, alpha, bg, hole = _t(*PS.inputs("soft", 4, 2, 24, 40, with_bg=True, with_hole=True))
    node = N.SDMatteCleanPlate()
    out, = node.fill(image, alpha, hole, bg, 0.5)
    assert eng.calls == [("fill_background", True, True, 0.5, False)] and out.device.type == "cpu"
    assert torch.equal(out, N.clean_plate(image, alpha, bg, hole, 0.5))
    eng.calls.clear()
    out, = node.fill(image, alpha[0:2], decontaminate=True)
    assert eng.calls == [("estimate_foreground", False), ("fill_background", True, False, 0.0625, False)]
    assert torch.equal(out, N.clean_plate(image, alpha, N.estimate_foreground(image, alpha)[1]))
    eng.calls.clear()
    node.fill(image, alpha, background=bg, decontaminate=True)
    assert eng.calls == [("fill_background", True, False, 0.0625, False)]


def test_plate_node_env_opt_in(pkg):
    """The module-level mappings follow SDMATTE_PLATE_NODE, independently of the other flags: a fresh interpreter each."""
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; p = load_package(); "
            "print(sorted(p.NODE_CLASS_MAPPINGS), sorted(p.NODE_DISPLAY_NAME_MAPPINGS))" % ROOT)
    flags = [k for k in os.environ if k.startswith("SDMATTE_") and k.endswith(("_NODE", "_NODES"))]
    for extra, plate, want in ((None, None, "['SDMatteApply']"), (None, "0", "['SDMatteApply']"), (None, "1", "['SDMatteApply', 'SDMatteCleanPlate']"),
                               ("1", "1", "['SDMatteApply', 'SDMatteApplyMask', 'SDMatteCleanPlate', 'SDMatteTrimapFromMask']"),
                               ("1", None, "['SDMatteApply', 'SDMatteApplyMask', 'SDMatteTrimapFromMask']")):
        env = {k: v for k, v in os.environ.items() if k not in flags}
        env.update({k: v for k, v in (("SDMATTE_EXTRA_NODES", extra), ("SDMATTE_PLATE_NODE", plate)) if v is not None})
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.strip() == f"{want} {want}", (extra, plate, r.stdout, r.stderr)


def test_product_library_exports_plate_call(pkg):
    """The gfx950 library exports the product call, and header, bindings and kernels agree on the defines, the three names and the launch formula."""
    from comfyui_sdmatte_amd import build, engine
    dll = ctypes.CDLL(build.build_all())
    assert "sdm_fill_background" in engine.EXPORTS
    getattr(dll, "sdm_fill_background")
    hdr = open(os.path.join(ROOT, "include", "sdmatte.h")).read()
    E = engine.Engine
    for line in (f"#define SDM_PLATE_ALPHA_CUT {E.PLATE_ALPHA_CUT}f\n", f"#define SDM_PLATE_MIN_CUT {E.PLATE_MIN_CUT}f\n"):
        assert line in hdr, line
    assert "1 + 2 * ceil(S / 3)" in hdr and all(f"`{k}`" in hdr for k in ("plate_pull", "plate_small", "plate_push"))
    src = open(os.path.join(ROOT, "comfyui-sdmatte_amd", "csrc", "sdm_engine.cpp")).read()
    assert all(src.count(f'count_kernel("{k}")') == 1 for k in ("plate_pull", "plate_small", "plate_push"))
    kern = open(os.path.join(ROOT, "comfyui-sdmatte_amd", "csrc", "k_plate.h")).read()
    assert "#define SDM_PLATE_SMALL 32 " in kern and "#define SDM_PLATE_GROUP 3 " in kern
    assert E.plate_launches(32, 32) == (0, 1, 0) and E.plate_launches(33, 31) == (1, 1, 1) and E.plate_launches(270, 480) == (2, 1, 2)
    assert E.plate_launches(2160, 3840) == (3, 1, 3)
