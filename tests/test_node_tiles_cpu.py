"""Tiled matting on the CPU: the grid rule (sdmatte_nodes.tile_axis), auto_tile, band_tiles against the brute force of tests/tiles_suite.py, blend_tiles, the
opt-in node SDMatteApplyTiled against a stub engine, and the mappings.  No GPU, no emulator."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def test_tile_axis_properties_over_a_sweep(pkg):
    """For T in {8, 16, 64, 100}, every O in 0 .. T/2 and every L up to 5T + 2: the first tile starts at 0, the last ends at L, the origins increase
    strictly, neighbours overlap by at least O, every pixel is covered, by at most three tiles."""
    from comfyui_sdmatte_amd.sdmatte_nodes import tile_axis
    import tiles_suite as TS
    most = 0
    for T in (8, 16, 64, 100):
        for O in range(T // 2 + 1):
            for L in range(1, 5 * T + 3):
                o, size = tile_axis(L, T, O)
                assert (o, size) == TS.axis(L, T, O)
                assert o[0] == 0 and o[-1] + size == L and size == min(L, T), (L, T, O)
                assert all(a < b for a, b in zip(o, o[1:])) and all(a + size - b >= O for a, b in zip(o, o[1:])), (L, T, O, o)
                cover = np.zeros(L, np.int64)
                for a in o:
                    cover[a:a + size] += 1
                assert cover.min() >= 1, (L, T, O)
                most = max(most, int(cover.max()))
    assert most == 3
    assert tile_axis(113, 64, 16) == ([0, 24, 49], 64)                                      # pixels 49 .. 63 lie in three tiles
    for bad in ((0, 64, 16), (100, 64, 33), (100, 64, -1), (100, 0, 0)):
        with pytest.raises(ValueError):
            tile_axis(*bad)


def test_auto_tile_examples(pkg):
    from comfyui_sdmatte_amd.sdmatte_nodes import auto_tile, tile_axis

    def cells(H, W, T, O):
        return len(tile_axis(H, T, O)[0]), len(tile_axis(W, T, O)[0])
    assert auto_tile(2160, 3840, 1024, 128) == 1024 and cells(2160, 3840, 1024, 128) == (3, 5)
    big = auto_tile(4320, 7680, 1024, 128)
    ny, nx = cells(4320, 7680, big, 128)
    assert big > 1024 and big % 64 == 0 and ny * nx <= 16
    py, px = cells(4320, 7680, big - 64, 128)
    assert py * px > 16                                                                      # the smallest such multiple
    assert auto_tile(500, 700, 1024, 128) == 1024 and auto_tile(500, 700, 1000, 128) == 1024 and auto_tile(96, 128, 64, 16, limit=4) == 128
    assert auto_tile(2160, 3840, 64, 100) == auto_tile(2160, 3840, 256, 100)                 # an overlap above half the tile grows the tile too
    with pytest.raises(ValueError):
        auto_tile(0, 10, 64, 0)


def test_band_tiles_restatement_equals_brute_force(pkg):
    import tiles_suite as TS
    from comfyui_sdmatte_amd.sdmatte_nodes import band_tiles
    TS.check_cases_mean_what_their_names_say()
    for name, plane, lo, hi, T, O, K in TS.band_cases():
        got, cnt = band_tiles(torch.from_numpy(plane), lo, hi, T, O, K, return_count=True)
        want, wcnt = TS.brute_force(plane, lo, hi, T, O, K)
        assert got.dtype == torch.int32 and cnt.dtype == torch.int32 and np.array_equal(got.numpy(), want) and np.array_equal(cnt.numpy(), wcnt), name
    p = torch.rand(1, 40, 50)
    for bad in (dict(band_lo=0.8), dict(band_hi=1.5), dict(tile=15), dict(overlap=513), dict(max_tiles=17), dict(max_tiles=0)):
        with pytest.raises(ValueError):
            band_tiles(p, **bad)
    with pytest.raises(ValueError):
        band_tiles(torch.rand(1, 150, 200), tile=16, overlap=8)
    assert band_tiles(torch.zeros(1, 6, 7), max_tiles=2).tolist() == [[[-1, 0, 0, 0, 0]] * 2]


def test_blend_tiles_single_coverage_is_exact_and_weights_sum_to_one(pkg):
    from comfyui_sdmatte_amd.sdmatte_nodes import band_tiles, blend_tiles, compact_boxes
    g = torch.Generator().manual_seed(3)
    H, W = 150, 200
    # disjoint tiles under a feather: every crop comes back bit for bit, the rest is the sanitised base
    tiles = torch.tensor([[0, 5, 8, 40, 48], [1, 50, 70, 40, 48], [-1, 0, 0, 0, 0], [0, 60, 100, 30, 20]], dtype=torch.int32)
    crops = [torch.rand(int(h), int(w), generator=g) for _, _, _, h, w in tiles.tolist()]
    base = torch.rand(2, H, W, generator=g) * 1.5 - 0.25
    base[0, 3, 3] = float("nan")
    out = blend_tiles(crops, tiles, 2, H, W, 7, base)
    want = torch.nan_to_num(base, nan=0.0).clamp(0, 1)
    for n, (b, y0, x0, h, w) in enumerate(tiles.tolist()):
        if b >= 0:
            assert torch.equal(out[b, y0:y0 + h, x0:x0 + w], crops[n])
            want[b, y0:y0 + h, x0:x0 + w] = crops[n]
    assert torch.equal(out, want) and out.dtype == torch.float32 and float(out[0, 3, 3]) == 0.0
    assert torch.equal(blend_tiles(crops, tiles, 2, H, W, 7)[0, 0], torch.zeros(W))         # no base: 0.0
    # every grid tile of a frame: constant crops stay the constant and the weights w_n / Wsum of every pixel sum to 1, within 2^-22 (up to nine quotients,
    # each rounded once: 9 * 2^-25 for the quotients and 8 * 2^-24 for the partial sums at most)
    from comfyui_sdmatte_amd.sdmatte_nodes import tile_axis
    for H, W, T, O, feather in ((150, 200, 64, 16, 16), (150, 200, 100, 50, 11), (150, 200, 80, 16, 0), (150, 200, 64, 16, 40), (113, 113, 64, 16, 16)):
        tl = compact_boxes(band_tiles(torch.full((1, H, W), 0.5), tile=T, overlap=O))
        assert tl.shape[0] == len(tile_axis(H, T, O)[0]) * len(tile_axis(W, T, O)[0]) <= 16
        ones = [torch.ones(int(h), int(w)) for _, _, _, h, w in tl.tolist()]
        s = blend_tiles(ones, tl, 1, H, W, feather)
        print(f"blend_tiles {H}x{W} T={T} O={O} feather={feather}: max |sum of weights - 1| {float((s - 1).abs().max()):.3g} (bound {2.0 ** -22:.3g})")
        assert float((s - 1).abs().max()) <= 2.0 ** -22 and float(s.max()) <= 1.0
        c = blend_tiles([0.375 * t for t in ones], tl, 1, H, W, feather)
        assert float((c - 0.375).abs().max()) <= 2.0 ** -22
    # two tiles side by side, feather 3: the ramp (d + 1) / 4 of the definition, the frame's border does not ramp
    two = torch.tensor([[0, 0, 0, 4, 10], [0, 0, 6, 4, 10]], dtype=torch.int32)
    out = blend_tiles([torch.zeros(4, 10), torch.ones(4, 10)], two, 1, 4, 16, 3)
    w0, w1 = [1.0, 0.75, 0.5, 0.25], [0.25, 0.5, 0.75, 1.0]
    want = torch.tensor([0.0] * 6 + [b / (a + b) for a, b in zip(w0, w1)] + [1.0] * 6)
    assert torch.allclose(out[0, 0], want, rtol=0, atol=2.0 ** -23) and torch.equal(out[0, 0], out[0, 3]), out[0, 0].tolist()
    for bad in ((crops[:2], tiles), (crops, torch.tensor([[0, 5, 8, 40, 48], [2, 50, 70, 40, 48], [-1, 0, 0, 0, 0], [0, 60, 100, 30, 20]]))):
        with pytest.raises(ValueError):
            blend_tiles(bad[0], bad[1], 2, 150, 200, 7, base)


class _StubEngine:
    """Records the apply_matte_tiles calls; make_trimap and band_tiles are the CPU restatements."""

    def __init__(self):
        self.calls = []

    def make_trimap(self, mask, threshold, erode_px, dilate_px):
        from comfyui_sdmatte_amd.sdmatte_nodes import trimap_from_mask
        return trimap_from_mask(mask, threshold, erode_px, dilate_px)

    def band_tiles(self, trimap, *args, return_count=False):
        from comfyui_sdmatte_amd.sdmatte_nodes import band_tiles
        return band_tiles(trimap, *args, return_count=return_count)

    def apply_matte_tiles(self, image, trimap, tiles, S, is_transparent, output_mode, mask_refine, trimap_constraint, feather_px, base):
        self.calls.append((tuple(image.shape), tiles.clone(), feather_px, base))
        B, H, W, _ = image.shape
        assert tiles.dtype == torch.int32 and 0 <= tiles.shape[0] <= 16 and (tiles.shape[0] == 0 or (int(tiles[:, 0].min()) >= 0 and int(tiles[:, 0].max()) < B))
        return torch.full((B, H, W), float(len(self.calls))), torch.zeros(B, H, W, 3)


def test_tiled_node_flow_against_a_stub_engine(pkg, monkeypatch):
    """B = 4: three images with a ring each and one without an unknown pixel: every call gets consecutive images with at most 16 entries in all, b
    rebased; a batch without any unknown pixel is one call with N = 0; the tiles come back per image as (x, y, width, height)."""
    import tiles_suite as TS
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    monkeypatch.setattr(N, "_trim_engine_memory", lambda model: None)

    class Model:
        pass
    model = Model()
    model.engine = _StubEngine()
    ringm = torch.from_numpy(np.where(TS.ring(150, 200) > 0.25, 1.0, 0.0).astype(np.float32))
    mask = torch.cat([ringm, ringm, torch.zeros(1, 150, 200), ringm])
    image = torch.rand(4, 150, 200, 3)
    base = torch.rand(4, 150, 200)
    a, m, t, tiles = N.SDMatteApplyTiled._run(model, image, mask, 0.5, 3, 3, 64, 16, 9, 0.25, 0.75, 64, False, "alpha_only", False, 0.8, base)
    per = [len(x) for x in tiles]
    assert per[2] == 0 and per[0] == per[1] == per[3] and 6 <= per[0] <= 12
    calls = model.engine.calls
    want_ranges, lo, n = [], 0, 0                                                            # split_boxes' rule: consecutive images, at most 16 entries
    for b in range(4):
        if n + per[b] > 16:
            want_ranges.append((lo, b))
            lo, n = b, 0
        n += per[b]
    want_ranges.append((lo, 4))
    assert len(want_ranges) >= 2
    assert [c[0][0] for c in calls] == [hi - lo for lo, hi in want_ranges] and all(c[2] == 9 for c in calls)
    assert sum(c[1].shape[0] for c in calls) == sum(per) and torch.equal(torch.cat([c[3] for c in calls]), base)
    assert a.shape == (4, 150, 200) and m.shape == (4, 150, 200, 3) and t.shape == (4, 150, 200)
    want, _ = TS.brute_force(t.numpy(), 0.25, 0.75, 64, 16, 16)
    assert tiles[3] == [(x0, y0, w, h) for _, y0, x0, h, w in want[3, :per[3]].tolist()]
    model.engine = _StubEngine()
    a, m, t, tiles = N.SDMatteApplyTiled._run(model, image[:2], torch.zeros(2, 150, 200), 0.5, 3, 3, 64, 16, 9, 0.25, 0.75, 64, False, "alpha_only", False, 0.8)
    assert tiles == [[], []] and len(model.engine.calls) == 1 and model.engine.calls[0][1].shape == (0, 5) and model.engine.calls[0][3] is None
    # more tiles than a call takes: refused with the way out
    model.engine = _StubEngine()
    stripes = torch.zeros(1, 150, 200)
    stripes[:, :, ::4] = 1.0                                                                 # every pixel within 3 of the other class: all unknown, 5 x 7 tiles of 32
    with pytest.raises(ValueError, match="tile_size"):
        N.SDMatteApplyTiled._run(model, image[:1], stripes, 0.5, 3, 3, 32, 0, 4, 0.25, 0.75, 64, False, "alpha_only", False, 0.8)


def test_with_tiled_node_and_input_types(pkg):
    """with_tiled_node adds exactly SDMatteApplyTiled and leaves its argument alone; node_mappings keeps its argument list."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    from comfyui_sdmatte_amd.engine import Engine
    assert "tiled" not in inspect.signature(N.node_mappings).parameters
    base = N.with_metrics_node(N.node_mappings(True), False)
    before = (dict(base[0]), dict(base[1]))
    assert N.with_tiled_node(base, False) == before
    classes, names = N.with_tiled_node(base)
    assert classes == dict(before[0], SDMatteApplyTiled=N.SDMatteApplyTiled) and names == dict(before[1], SDMatteApplyTiled="Apply SDMatte (Tiled)")
    assert (base[0], base[1]) == before
    f = N.SDMatteApplyTiled
    it = f.INPUT_TYPES()
    mask_it = N.SDMatteApplyMask.INPUT_TYPES()
    new = ["tile_size", "overlap", "feather", "band_lo", "band_hi"]
    req = it["required"]
    assert [k for k in req if k not in new] == list(mask_it["required"]) and all(req[k] == mask_it["required"][k] for k in mask_it["required"])
    assert [k for k in req if k in new] == new
    assert list(it["optional"]) == list(mask_it["optional"]) + ["base_alpha"] and it["optional"]["base_alpha"][0] == "MASK"
    defaults = {k: v.default for k, v in inspect.signature(Engine.band_tiles).parameters.items() if v.default is not inspect.Parameter.empty}
    assert req["tile_size"][1]["default"] == 0 and req["overlap"][1]["default"] == defaults["overlap"]
    assert req["band_lo"][1]["default"] == defaults["band_lo"] and req["band_hi"][1]["default"] == defaults["band_hi"]
    assert req["feather"][1]["max"] == Engine.TILES_MAX_FEATHER
    assert {k: v.default for k, v in inspect.signature(N.band_tiles).parameters.items() if k in defaults} == {
        k: v for k, v in defaults.items() if k in inspect.signature(N.band_tiles).parameters}
    assert f.RETURN_TYPES == ("MASK", "IMAGE", "MASK", "BBOX") and f.RETURN_NAMES[-1] == "tiles" and f.CATEGORY == "Matting/SDMatte"
    assert list(inspect.signature(getattr(f, f.FUNCTION)).parameters) == ["self"] + list(req) + list(it["optional"])
    # input validation comes before any model is looked for
    img, msk = torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8)
    tail = (64, False, "alpha_only", True, 0.8)
    for bad in ((img[..., :2], msk, 0.5, 1, 1, 0, 16, -1, 0.25, 0.75), (img, msk[:, :4], 0.5, 1, 1, 0, 16, -1, 0.25, 0.75), (img, msk, 0.5, 1, 1, 0, 16, -1, 0.8, 0.75),
                (img, msk, 0.5, 1, 1, 8, 0, -1, 0.25, 0.75), (img, msk, 0.5, 1, 1, 64, 33, -1, 0.25, 0.75), (img, msk, 0.5, 1, 1, 64, 16, 1025, 0.25, 0.75)):
        with pytest.raises(ValueError):
            f().apply_matte("SDMatte.safetensors", *bad, *tail)
    with pytest.raises(ValueError):
        f().apply_matte("SDMatte.safetensors", img, msk, 0.5, 1, 1, 0, 16, -1, 0.25, 0.75, *tail, base_alpha=msk[:, :4])
    with pytest.raises(RuntimeError, match="force_cpu"):
        f().apply_matte("SDMatte.safetensors", img, msk, 0.5, 1, 1, 0, 16, -1, 0.25, 0.75, *tail, force_cpu=True)


def test_tiled_node_env_opt_in(pkg):
    """The module-level mappings follow SDMATTE_TILED_NODE, independently of the other flags: a fresh interpreter each."""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; p = load_package(); "
            "print(sorted(p.NODE_CLASS_MAPPINGS), sorted(p.NODE_DISPLAY_NAME_MAPPINGS))" % ROOT)
    flags = [k for k in os.environ if k.startswith("SDMATTE_") and k.endswith(("_NODE", "_NODES"))]
    for extra, tiled, want in ((None, None, "['SDMatteApply']"), (None, "0", "['SDMatteApply']"), (None, "1", "['SDMatteApply', 'SDMatteApplyTiled']"),
                               ("1", "1", "['SDMatteApply', 'SDMatteApplyMask', 'SDMatteApplyTiled', 'SDMatteTrimapFromMask']"),
                               ("1", None, "['SDMatteApply', 'SDMatteApplyMask', 'SDMatteTrimapFromMask']")):
        env = {k: v for k, v in os.environ.items() if k not in flags}
        env.update({k: v for k, v in (("SDMATTE_EXTRA_NODES", extra), ("SDMATTE_TILED_NODE", tiled)) if v is not None})
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.strip() == f"{want} {want}", (extra, tiled, r.stdout, r.stderr)


def test_product_library_exports_tiles_calls(pkg):
    """The gfx950 library exports the two new product calls, and header and bindings agree on the limits."""
    from comfyui_sdmatte_amd import build, engine
    dll = ctypes.CDLL(build.build_all())
    for name in ("sdm_band_tiles", "sdm_apply_matte_tiles"):
        assert name in engine.EXPORTS
        getattr(dll, name)
    hdr = open(os.path.join(ROOT, "include", "sdmatte.h")).read()
    E = engine.Engine
    assert f"#define SDM_TILES_MAX {E.TILES_MAX} " in hdr and f"#define SDM_TILES_MAX_GRID {E.TILES_MAX_GRID}\n" in hdr
    assert f"#define SDM_TILES_MAX_FEATHER {E.TILES_MAX_FEATHER}\n" in hdr and E.TILES_MAX == E.BOXES_MAX_TOTAL
