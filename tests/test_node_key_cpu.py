"""The CPU side of the green-screen calls: the numpy reference of tests/key_suite.py on its own (fp32 against fp64, the purpose scene), the torch
restatement (sdmatte_nodes.screen_colour / chroma_key / key_screen) against it, the two opt-in nodes, and the agreement of header, bindings and library.
No GPU, no emulator."""
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


def test_reference_fp32_distance_and_case_list(pkg):
    """On the reference alone: the colour's fp32 variants stay within 1e-6 of fp64; the fp32 key stays within 1e-5 of the fp64 key wherever both see the
    same side of every compare; the list holds the sizes, hints, shared slots and kinds the kernels branch on."""
    import key_suite as KS
    from comfyui_sdmatte_amd.engine import Engine
    # the suite's constants are the package's
    assert KS.DEFAULTS == tuple(Engine.KEY_DEFAULTS.values()) and KS.OUTPUTS == Engine.KEY_OUTPUTS and KS.COLOUR_LAUNCHES == tuple(Engine.SCREEN_COLOUR_LAUNCHES)
    assert (float(KS.MIN_SUM), float(KS.MIN_SAT), float(KS.MIN_SEP), KS.RUN) == tuple(np.float32(v) for v in (Engine.KEY_MIN_SUM, Engine.KEY_MIN_SAT, Engine.KEY_MIN_SEP)) + (Engine.KEY_RUN, )
    assert {v: k for k, v in Engine.KEY_HINTS.items()} == KS.HINT_NAMES
    shapes = {c[2:5] for c in KS.CASES}
    assert shapes == {(1, 1, 1), (1, 3, 5), (2, 9, 37), (3, 67, 130), (2, 64, 256), (1, 130, 260)}
    assert {c[5] for c in KS.CASES} == {0, 1, 2} and {c[6] for c in KS.CASES} == {0, 1} and {c[1] for c in KS.CASES} == set(KS.KINDS)
    assert KS.RADII == ((0, 0), (1, 3), (10, 10)) and KS.BIG_RADIUS_CASE[2:5] == (1, 40, 70)
    plan = KS.key_plan()
    assert {p[3] for p in plan} >= {("key", ), ("trimap", ), ("despilled", ), KS.OUTPUTS} and plan[-1][2] == (255, 255)
    for name, *_ in KS.CASES:
        c64, info, d32 = KS.colour_refs(name)
        print(f"[key] {name}: info = {info[0].tolist()} d32 = {d32:.3e} tol = {KS.tolerance(d32):.3e}")
        assert d32 <= 1e-6, name
        assert (info[:, 0] >= info[:, 1]).all() and ((info[:, 1] > 0) == (info[:, 2] >= 0)).all()
    assert KS.colour_refs("grey_1x3x5_green")[1].tolist() == [[0, 0, -1, -1]] and not KS.colour_refs("grey_1x3x5_green")[0].any()
    assert KS.colour_refs("flat_2x64x256_green")[1].tolist() == [[16384, 16384, 6, 41]] * 2      # one colour in bin (7, 42): nine equal sums, the smallest index
    img, colour = KS.case_image("screen_1x130x260_green"), KS.case_screens("screen_1x130x260_green")[0]
    r32, r64 = KS.key_reference(img, colour, KS.DEFAULTS), KS.key_reference(img, colour, KS.DEFAULTS, np.float64)
    agree = r32["cls"] == r64["cls"]
    assert agree.mean() > 0.999 and float(np.abs(r32["key"] - r64["key"]).max()) <= 1e-5
    assert float(np.abs(r32["despilled"] - r64["despilled"]).max()) <= 1e-6


def test_reference_meets_the_purpose(pkg):
    """The conditions of the purpose scene hold for the reference at erode = dilate = 16, with the figures of the suite's docstring; a key that calls the
    whole frame subject fails them."""
    import key_suite as KS
    from comfyui_sdmatte_amd.engine import Engine
    assert KS.PURPOSE_CUT == Engine.KEY_SCREEN_CUT                      # the scene is measured at the two-pass call's default cut
    one, two = KS.purpose_reference()
    assert one[:2] == (0, 0) and two[:2] == (0, 0)
    assert abs(one[2] - 0.5405) < 5e-4 and abs(two[2] - 0.2299) < 5e-4 and abs(one[3] - 0.0358) < 5e-4 and abs(two[3] - 0.0127) < 5e-4
    img, alpha = KS.purpose_scene()
    with pytest.raises(AssertionError):
        bad = KS.purpose_figures(np.ones_like(alpha), np.ones_like(alpha), alpha)
        KS._assert_purpose("all subject", bad, bad, img)


def test_restatement_case_list(pkg):
    import key_suite as KS
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    KS.check_colour(N.screen_colour, lambda t: t)
    KS.check_key(N.chroma_key, lambda t: t)
    # fp64 is the reference in fp64: the colour to rounding, the key exactly
    for name, _, _, _, _, hint, share in KS.CASES:
        c = N.screen_colour(torch.from_numpy(KS.case_image(name).copy()), KS.HINT_NAMES[hint], bool(share), dtype=torch.float64)
        c64 = KS.colour_refs(name)[0]
        fin = np.isfinite(c64)
        assert c.dtype == torch.float64 and np.array_equal(np.isfinite(c.numpy()), fin) and float(np.abs(c.numpy() - c64)[fin].max(initial=0.0)) <= 1e-12, name
    img, (colour, plane) = KS.case_image("dirty_3x67x130_green"), KS.case_screens("dirty_3x67x130_green")
    for screen in (colour, plane):
        got = N.chroma_key(torch.from_numpy(img.copy()), torch.from_numpy(screen), *KS.DEFAULTS, dtype=torch.float64)
        ref = KS.key_reference(img, screen, KS.DEFAULTS, np.float64)
        assert all(g.dtype == torch.float64 and np.array_equal(g.numpy(), ref[w], equal_nan=True) for g, w in zip(got, KS.OUTPUTS))


def test_restatement_purpose_and_identities(pkg):
    """What the header states bit for bit holds for the restatement too; key_screen is the chain."""
    import key_suite as KS
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    KS.check_identities(N.screen_colour, N.chroma_key, lambda t: t, "torch restatement")
    KS.check_trimap_formula(N.chroma_key, N.trimap_from_mask, lambda t: t, "torch restatement")
    KS.check_purpose(N.screen_colour, N.chroma_key, N.clean_plate, lambda t: t, "torch restatement", N.key_screen)


def test_argument_checks(pkg):
    """ValueError from the restatement (the limits are those of Engine.chroma_key), and the Python defaults the issue names."""
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.sdmatte_nodes import chroma_key, key_screen, screen_colour
    img, colour = torch.rand(2, 10, 12, 3), torch.tensor([[0.1, 0.8, 0.2], [0.1, 0.7, 0.3]])
    nan, inf = float("nan"), float("inf")
    for kw in ({"clip_fg": -0.1}, {"clip_fg": 1.0}, {"clip_fg": nan}, {"clip_bg": 0.15}, {"clip_bg": 1.5}, {"clip_bg": nan}, {"sure_fg": -1.5},
               {"sure_fg": inf}, {"sure_bg": 0.0}, {"sure_bg": 2.5}, {"despill": -0.1}, {"despill": 1.5}, {"despill": "1"}, {"erode_px": -1},
               {"dilate_px": 256}, {"erode_px": 0.5}, {"want": ()}, {"want": ("key", "alpha")}, {"dtype": torch.float16}):
        with pytest.raises(ValueError):
            chroma_key(img, colour, **kw)
    for bad in ((img[..., :2], colour), (img, colour[:1]), (img, img[:, :5]), (img[0], colour)):
        with pytest.raises(ValueError):
            chroma_key(*bad)
    for kw in ({"hint": "red"}, {"hint": 3}, {"dtype": torch.float16}):
        with pytest.raises(ValueError):
            screen_colour(img, **kw)
    with pytest.raises(ValueError):
        key_screen(img, screen_cut=0.0)
    assert chroma_key(img, colour, clip_fg=0.0, clip_bg=1.0, sure_fg=-1.0, sure_bg=2.0, erode_px=255, dilate_px=0, despill=0.0, want="key").shape == (2, 10, 12)
    assert chroma_key(img, colour.view(2, 1, 1, 3), want="despilled").shape == img.shape and screen_colour(img, 2).shape == (2, 3)
    want = {"clip_fg": 0.15, "clip_bg": 0.85, "sure_fg": 0.05, "sure_bg": 0.95, "erode_px": 10, "dilate_px": 10, "despill": 1.0}
    assert Engine.KEY_DEFAULTS == want and Engine.KEY_HINTS == {"any": 0, "green": 1, "blue": 2}
    for fn in (Engine.chroma_key, chroma_key, Engine.key_screen, key_screen):
        d = {k: v.default for k, v in inspect.signature(fn).parameters.items() if k in want}
        assert d == want, fn
        assert inspect.signature(fn).parameters["want"].default == ("key", "trimap", "despilled")
    d = {k: v.default for k, v in inspect.signature(Engine.screen_colour).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == {"hint": "green", "share": False, "return_info": False, "sync": True}
    d = inspect.signature(Engine.key_screen).parameters
    assert d["screen_correction"].default is True and d["screen_cut"].default == 0.25 and d["sync"].default is True


def test_with_key_nodes(pkg):
    """with_key_nodes adds exactly the two nodes and does not modify its argument; node_mappings keeps its signature; the nodes' inputs match their
    functions."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    base = N.with_plate_node(N.node_mappings(True), True)
    before = (dict(base[0]), dict(base[1]))
    classes, names = N.with_key_nodes(base)
    assert base == before and N.with_key_nodes(base, False) == before
    assert classes == dict(before[0], SDMatteChromaKey=N.SDMatteChromaKey, SDMatteDespill=N.SDMatteDespill)
    assert names == dict(before[1], SDMatteChromaKey="SDMatte Chroma Key (Green Screen)", SDMatteDespill="SDMatte Despill")
    assert list(inspect.signature(N.with_key_nodes).parameters) == ["mappings", "on"]
    assert list(inspect.signature(N.node_mappings).parameters)[:2] == ["extra", "foreground"] and "key" not in inspect.signature(N.node_mappings).parameters
    for f in (N.SDMatteChromaKey, N.SDMatteDespill):
        it = f.INPUT_TYPES()
        assert f.CATEGORY == "Matting/SDMatte"
        assert list(inspect.signature(getattr(f, f.FUNCTION)).parameters) == ["self"] + list(it["required"]) + list(it["optional"])
        assert it["optional"]["force_cpu"][1]["default"] is False and all(spec[1]["tooltip"] for spec in it["optional"].values())
        fn_defaults = {k: v.default for k, v in inspect.signature(getattr(f, f.FUNCTION)).parameters.items() if v.default is not inspect.Parameter.empty}
        assert fn_defaults == {k: spec[1]["default"] for k, spec in it["optional"].items()}
    f = N.SDMatteChromaKey
    assert f.RETURN_TYPES == ("MASK", "MASK", "IMAGE", "IMAGE") and f.RETURN_NAMES == ("trimap", "key", "despilled", "screen")
    assert N.SDMatteDespill.RETURN_TYPES == ("IMAGE", ) and N.SDMatteDespill.INPUT_TYPES()["required"]["screen"][0] == "IMAGE"
    assert "SDMATTE_KEY_NODES=1" in N.__doc__


def test_nodes_cpu_path_equals_restatement(pkg):
    """force_cpu=True is the restatement, argument by argument; the screen leaves as an IMAGE ([B,1,1,3], or the plate) that SDMatteDespill takes back."""
    import key_suite as KS
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    img = torch.from_numpy(KS.inputs("screen", 2, 2, 24, 40))
    node, desp_node = N.SDMatteChromaKey(), N.SDMatteDespill()
    tri, key, desp, screen = node.key(img, force_cpu=True)
    want = N.key_screen(img, want=("trimap", "key", "despilled"))
    assert screen.shape == img.shape and all(torch.equal(a, b) for a, b in zip((tri, key, desp, screen), want))
    tri, key, desp, screen = node.key(img, "green", True, False, 0.25, 0.1, 0.9, 0.0, 1.0, 2, 3, 0.5, force_cpu=True)
    want = N.key_screen(img, "green", True, False, 0.25, 0.1, 0.9, 0.0, 1.0, 2, 3, 0.5, want=("trimap", "key", "despilled"))
    assert screen.shape == (2, 1, 1, 3) and torch.equal(screen.view(2, 3), want[3]) and all(torch.equal(a, b) for a, b in zip((tri, key, desp), want))
    assert torch.equal(screen[0], screen[1])                             # share: one screen for the clip
    out, = desp_node.despill(img, screen, 0.5, force_cpu=True)
    assert torch.equal(out, desp) and torch.equal(out, N.chroma_key(img, screen, despill=0.5, want="despilled"))
    plate = node.key(img, force_cpu=True)[3]
    out, = desp_node.despill(img, plate, force_cpu=True)
    assert torch.equal(out, N.chroma_key(img, plate, want="despilled"))
    for bad in ((img[..., :2], ), (img[0], )):
        with pytest.raises(ValueError):      # input validation comes before any engine is looked for
            node.key(*bad)
    for bad in ((img[..., :2], screen), (img, screen[:1]), (img, screen.view(2, 3))):
        with pytest.raises(ValueError):
            desp_node.despill(*bad)


class _StubEngine:
    """Engine.key_screen / chroma_key by their restatements, with a record of the calls."""

    def __init__(self):
        self.calls = []

    def key_screen(self, image, *args, sync=True):
        from comfyui_sdmatte_amd.sdmatte_nodes import key_screen
        self.calls.append(("key_screen", args, sync))
        return key_screen(image, *args)

    def chroma_key(self, image, screen, despill=1.0, want=("key", "trimap", "despilled"), sync=True):
        from comfyui_sdmatte_amd.sdmatte_nodes import chroma_key
        self.calls.append(("chroma_key", tuple(screen.shape), despill, want, sync))
        return chroma_key(image, screen, despill=despill, want=want)


def test_nodes_engine_path_against_a_stub_engine(pkg, monkeypatch):
    """Without force_cpu each node makes one engine call without a sync and returns CPU tensors."""
    import key_suite as KS
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    eng = _StubEngine()
    monkeypatch.setattr(N, "_torch_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(N, "_trimap_engine", lambda device: eng)
    img = torch.from_numpy(KS.inputs("screen", 4, 2, 24, 40))
    got = N.SDMatteChromaKey().key(img, "any", False, True, 0.5, erode_px=3, dilate_px=4)
    args = ("any", False, True, 0.5, 0.15, 0.85, 0.05, 0.95, 3, 4, 1.0, ("trimap", "key", "despilled"))
    assert eng.calls == [("key_screen", args, False)] and all(t.device.type == "cpu" for t in got)
    assert all(torch.equal(a, b) for a, b in zip(got, N.key_screen(img, *args)))
    eng.calls.clear()
    screen = got[3]
    out, = N.SDMatteDespill().despill(img, screen, 0.25)
    assert eng.calls == [("chroma_key", (2, 24, 40, 3), 0.25, ("despilled", ), False)]
    assert torch.equal(out, N.chroma_key(img, screen, despill=0.25, want="despilled"))


def test_key_nodes_env_opt_in(pkg):
    """The module-level mappings follow SDMATTE_KEY_NODES, independently of the other flags: a fresh interpreter each."""
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; p = load_package(); "
            "print(sorted(p.NODE_CLASS_MAPPINGS), sorted(p.NODE_DISPLAY_NAME_MAPPINGS))" % ROOT)
    flags = [k for k in os.environ if k.startswith("SDMATTE_") and k.endswith(("_NODE", "_NODES"))]
    for extra, key, want in ((None, None, "['SDMatteApply']"), (None, "0", "['SDMatteApply']"),
                             (None, "1", "['SDMatteApply', 'SDMatteChromaKey', 'SDMatteDespill']"),
                             ("1", "1", "['SDMatteApply', 'SDMatteApplyMask', 'SDMatteChromaKey', 'SDMatteDespill', 'SDMatteTrimapFromMask']"),
                             ("1", None, "['SDMatteApply', 'SDMatteApplyMask', 'SDMatteTrimapFromMask']")):
        env = {k: v for k, v in os.environ.items() if k not in flags}
        env.update({k: v for k, v in (("SDMATTE_EXTRA_NODES", extra), ("SDMATTE_KEY_NODES", key)) if v is not None})
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.strip() == f"{want} {want}", (extra, key, r.stdout, r.stderr)


def test_product_library_exports_key_calls(pkg):
    """The gfx950 library exports both calls, and header, bindings and kernels agree on the defines and the launch names."""
    from comfyui_sdmatte_amd import build, engine
    dll = ctypes.CDLL(build.build_all())
    for name in ("sdm_screen_colour", "sdm_chroma_key"):
        assert name in engine.EXPORTS
        getattr(dll, name)
    hdr = open(os.path.join(ROOT, "include", "sdmatte.h")).read()
    E = engine.Engine
    d = E.KEY_DEFAULTS
    for line in (f"#define SDM_KEY_MIN_SUM {E.KEY_MIN_SUM}f\n", f"#define SDM_KEY_MIN_SAT {E.KEY_MIN_SAT}f\n", f"#define SDM_KEY_MIN_SEP {E.KEY_MIN_SEP}f\n",
                 f"#define SDM_KEY_RUN {E.KEY_RUN}\n", f"#define SDM_KEY_MAX_SLOTS {E.KEY_MAX_SLOTS}\n", f"#define SDM_KEY_CLIP_FG {d['clip_fg']}f\n", f"#define SDM_KEY_CLIP_BG {d['clip_bg']}f\n",
                 f"#define SDM_KEY_SURE_FG {d['sure_fg']}f\n", f"#define SDM_KEY_SURE_BG {d['sure_bg']}f\n"):
        assert line in hdr, line
    names = tuple(E.SCREEN_COLOUR_LAUNCHES) + ("ck_key", "ck_veto")
    assert all(f"`{k}`" in hdr for k in names + ("trimap_cols", "trimap_rows"))
    src = open(os.path.join(ROOT, "comfyui-sdmatte_amd", "csrc", "sdm_engine.cpp")).read()
    assert all(src.count(f'count_kernel("{k}")') == 1 for k in names)
    kern = open(os.path.join(ROOT, "comfyui-sdmatte_amd", "csrc", "k_key.h")).read()
    assert all(f"void {k}_kernel(" in kern for k in names)
    assert "#define SDM_KEY_RUN_PX 4096 " in kern and "#define SDM_KEY_HIST_PX 16384 " in kern and "#define SDM_KEY_BINS 64 " in kern
    assert E.key_launches(("key", )) == {"ck_key": 1} and sum(E.key_launches().values()) == 4 and sum(E.SCREEN_COLOUR_LAUNCHES.values()) == 5
