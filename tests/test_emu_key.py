"""Green-screen calls on the kernel emulator: the kernels of csrc/k_key.h (both load paths, the wave's one-bin shortcut of ck_hist, ragged runs, shared
slots) and the unchanged trimap kernels behind them, through sdm_screen_colour and sdm_chroma_key with host pointers, on an engine that never loaded
weights.  The real-kernel versions are tests/test_gpu_key.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _emu_engine():
    from emu.build_emu import build
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Bindings, Engine
    return Engine(SDMatteConfig.tiny(), 0, True, _lib=Bindings(ctypes.CDLL(build())), precision="fp16")


@pytest.fixture(scope="module")
def emu(pkg):
    eng = _emu_engine()
    yield eng
    eng.close()


def test_emu_screen_colour_case_list(emu):
    """Every case: info exactly, the colour under the suite's rule; five launches per call."""
    import key_suite as KS
    emu.lib.kernel_counts(reset=True)
    n = KS.check_colour(emu.screen_colour, lambda t: t)
    assert emu.lib.kernel_counts() == {k: n for k in KS.COLOUR_LAUNCHES}


def test_emu_chroma_key_case_list(emu):
    """Every entry of the plan (the 255-pixel radii at 1x40x70 included: a second here) bit for bit against the fp32 reference; the launches of the
    whole run are the documented ones per call."""
    import key_suite as KS
    emu.lib.kernel_counts(reset=True)
    plan = KS.check_key(emu.chroma_key, lambda t: t)
    assert emu.lib.kernel_counts() == KS.key_launches(plan)


def test_emu_key_identities(emu):
    import key_suite as KS
    KS.check_identities(emu.screen_colour, emu.chroma_key, lambda t: t, "emulator")
    KS.check_trimap_formula(emu.chroma_key, emu.make_trimap, lambda t: t, "emulator")


def test_emu_key_load_paths_agree(emu):
    """Identity 6, alignment: tensors that start 4 bytes off a 16-byte boundary (scalar loads and stores) give the bits of the aligned ones."""
    import key_suite as KS
    for H, W in ((64, 256), (9, 37)):
        img = torch.from_numpy(KS.inputs("dirty", H, 2, H, W))
        colour, info = emu.screen_colour(img, "green", return_info=True)
        plane = torch.from_numpy(KS.inputs("screen", W, 2, H, W))
        assert img.data_ptr() % 16 == 0 and plane.data_ptr() % 16 == 0
        off_img, off_plane = KS.offset_copy(img), KS.offset_copy(plane)
        c2, i2 = emu.screen_colour(off_img, "green", return_info=True)
        assert KS.same_bits(colour, c2) and torch.equal(info, i2), (H, W)
        ref = emu.chroma_key(img, plane, erode_px=2, dilate_px=3)
        for a, b in ((off_img, plane), (img, off_plane), (off_img, off_plane)):
            assert all(KS.same_bits(x, y) for x, y in zip(ref, emu.chroma_key(a, b, erode_px=2, dilate_px=3))), (H, W)


@pytest.mark.parametrize("H,W", [(9, 37), (64, 256)])
def test_emu_key_launches_per_output_combination(emu, H, W):
    """1 launch without the trimap, 4 with it, 5 for the colour: a function of the arguments only."""
    import key_suite as KS
    img = torch.from_numpy(KS.inputs("screen", 3, 2, H, W))
    for share in (False, True):
        emu.lib.kernel_counts(reset=True)
        colour = emu.screen_colour(img, "green", share)
        assert emu.lib.kernel_counts() == emu.SCREEN_COLOUR_LAUNCHES == {k: 1 for k in KS.COLOUR_LAUNCHES}
    for want in (("key", ), ("trimap", ), ("despilled", ), ("key", "trimap"), ("key", "despilled"), ("trimap", "despilled"), KS.OUTPUTS):
        emu.lib.kernel_counts(reset=True)
        emu.chroma_key(img, colour, want=want)
        assert emu.lib.kernel_counts() == emu.key_launches(want) == KS.key_launches([(None, None, None, want)]), want
    # the trimap without the key equals the trimap with it (the key then lives in the arena)
    assert torch.equal(emu.chroma_key(img, colour, want="trimap"), emu.chroma_key(img, colour, want=("key", "trimap"))[1])


def test_emu_key_serves_its_purpose(emu):
    import key_suite as KS
    KS.check_purpose(emu.screen_colour, emu.chroma_key, emu.fill_background, lambda t: t, "emulator", emu.key_screen)


def test_emu_key_argument_checks_and_memory(emu):
    """Every parameter bound on both sides: ValueError from Python, SDM_ERR_INVALID with the argument's name from the C ABI, the outputs untouched and
    nothing queued or allocated; what a call keeps is counted by resident_bytes and given back by release_memory."""
    from comfyui_sdmatte_amd.engine import _ptr
    img, colour = torch.rand(2, 20, 36, 3), torch.tensor([[0.1, 0.8, 0.2], [0.1, 0.7, 0.3]])
    nan, inf = float("nan"), float("inf")
    bad = ({"clip_fg": -0.1}, {"clip_fg": 1.0}, {"clip_fg": nan}, {"clip_bg": 0.15}, {"clip_bg": 0.1}, {"clip_bg": 1.5}, {"clip_bg": nan},
           {"sure_fg": -1.5}, {"sure_fg": 1.5}, {"sure_fg": inf}, {"sure_bg": 0.0}, {"sure_bg": 2.5}, {"sure_bg": nan}, {"despill": -0.1},
           {"despill": 1.5}, {"despill": nan}, {"erode_px": -1}, {"dilate_px": 256}, {"erode_px": 1.5})
    for kw in bad:
        with pytest.raises(ValueError):
            emu.chroma_key(img, colour, **kw)
    for args, kw in (((img[..., :2], colour), {}), ((img, colour[:1]), {}), ((img, img[:, :5]), {}), ((img[0], colour), {}), ((img, colour), {"want": ()}),
                     ((img, colour), {"want": ("key", "key")}), ((img, colour), {"want": ("alpha", )})):
        with pytest.raises(ValueError):
            emu.chroma_key(*args, **kw)
    for kw in ({"hint": "red"}, {"hint": 3}):
        with pytest.raises(ValueError):
            emu.screen_colour(img, **kw)
    with pytest.raises(ValueError):
        emu.screen_colour(img[0])
    many = torch.rand(emu.KEY_MAX_SLOTS + 1, 1, 1, 3)                    # a histogram per image: bounded without share, one slot with it
    with pytest.raises(ValueError):
        emu.screen_colour(many)
    assert emu.screen_colour(many, "any", share=True).shape == (emu.KEY_MAX_SLOTS + 1, 3)
    with pytest.raises(ValueError):
        emu.key_screen(img, screen_cut=0.0)
    emu.release_memory()
    key, tri, desp = torch.full((2, 20, 36), -7.0), torch.full((2, 20, 36), -7.0), torch.full((2, 20, 36, 3), -7.0)
    scr, info = torch.full((2, 3), -7.0), torch.full((2, 4), -7, dtype=torch.int32)

    def raw_key(B=2, H=20, W=36, plane=0, cf=0.15, cb=0.85, sf=0.05, sb=0.95, e=10, d=10, ds=1.0, outs=(key, tri, desp), kind=0):
        return emu.lib.sdm_chroma_key(emu.h, _ptr(img), _ptr(colour), plane, B, H, W, cf, cb, sf, sb, e, d, ds, *(_ptr(o) for o in outs), kind, None)

    def raw_colour(B=2, H=20, W=36, hint=1, share=0, kind=0):
        return emu.lib.sdm_screen_colour(emu.h, _ptr(img), B, H, W, hint, share, _ptr(scr), _ptr(info), kind, None)
    emu.lib.kernel_counts(reset=True)
    err = lambda: emu.lib.sdm_last_error(emu.h)
    for kw, name in (({"cf": -0.1}, b"clip_fg"), ({"cf": 1.0}, b"clip_fg"), ({"cf": nan}, b"clip_fg"), ({"cb": 0.15}, b"clip_bg"), ({"cb": 1.5}, b"clip_bg"),
                     ({"cb": nan}, b"clip_bg"), ({"sf": -1.5}, b"sure_fg"), ({"sf": inf}, b"sure_fg"), ({"sb": 0.0}, b"sure_bg"), ({"sb": 2.5}, b"sure_bg"),
                     ({"sb": nan}, b"sure_bg"), ({"ds": -0.1}, b"despill"), ({"ds": 1.5}, b"despill"), ({"ds": nan}, b"despill"), ({"e": -1}, b"chroma key: erode_px"),
                     ({"d": 256}, b"chroma key: erode_px"), ({"d": 256, "outs": (key, None, desp)}, b"dilate_px"), ({"plane": 2}, b"screen_is_plane"), ({"outs": (None, None, None)}, b"at least one"),
                     ({"H": 0}, b"bad image size"), ({"B": 0}, b"bad image size"), ({"W": 32769}, b"too large"), ({"kind": 2}, b"ptr_kind")):
        assert raw_key(**kw) == -1 and name in err(), (kw, err())
    for kw, name in (({"hint": 3}, b"hint"), ({"hint": -1}, b"hint"), ({"share": 2}, b"share"), ({"B": 65537, "H": 1, "W": 1}, b"too large without share"), ({"W": 0}, b"bad image size"), ({"H": 32769}, b"too large"),
                     ({"kind": 2}, b"ptr_kind")):
        assert raw_colour(**kw) == -1 and name in err(), (kw, err())
    assert emu.lib.kernel_counts() == {} and emu.resident_bytes() == emu.weight_bytes()
    assert all(bool((t == -7).all()) for t in (key, tri, desp, scr, info))       # nothing queued, allocated or written
    assert raw_colour() == 0 and raw_key() == 0
    c2, i2 = emu.screen_colour(img, "green", return_info=True)
    assert torch.equal(scr, c2) and torch.equal(info, i2)
    assert all(torch.equal(a, b) for a, b in zip((key, tri, desp), emu.chroma_key(img, colour)))
    # host pointers: the staging (3 floats per pixel in, 1 + 1 + 3 out) and, in the arena, a class byte and an int16 per pixel
    assert emu.resident_bytes() >= emu.weight_bytes() + 2 * 20 * 36 * (12 + 20 + 3)
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    assert raw_colour() == 0                                             # ... the image in, and a histogram slot per image in the arena
    assert emu.resident_bytes() >= emu.weight_bytes() + 2 * 20 * 36 * 12 + 2 * 4096 * 4
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
