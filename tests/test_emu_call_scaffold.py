"""The call scaffold that every product call shares (product_call in csrc/sdm_engine.cpp: pointer kinds, I/O staging, the two arena passes), on the
kernel emulator and through the raw C ABI where `Engine` would stop the call first.  What each call computes is the business of
test_emu_{trimap,foreground,guided,e2e}.py; here the calls are compared with themselves on a fresh engine."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

HOST, DEVICE, INVALID = 0, 1, -1      # sdm_ptr_kind, SDM_ERR_INVALID (include/sdmatte.h); the emulator's "device" memory is host memory
SENTINEL = -7.0


def _emu_engine(cfg=None):
    from emu.build_emu import build
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Bindings, Engine
    return Engine(cfg or SDMatteConfig.tiny(), 0, True, _lib=Bindings(ctypes.CDLL(build())), precision="fp16")


def _rand(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def _out(*shape):
    return torch.full(shape, SENTINEL)


# each: (engine, ptr_kind, ...) -> (rc, outputs); the outputs start as SENTINEL
def _make_trimap(eng, kind, mask, erode_px=3, dilate_px=5):
    from comfyui_sdmatte_amd.engine import _ptr
    B, H, W = mask.shape
    out = _out(B, H, W)
    return eng.lib.sdm_make_trimap(eng.h, _ptr(mask), B, H, W, 0.5, erode_px, dilate_px, _ptr(out), kind, None), (out,)


def _estimate_foreground(eng, kind, image, alpha, fg_channels=3, want_bg=True):
    from comfyui_sdmatte_amd.engine import _ptr
    B, H, W, _ = image.shape
    fg, bg = _out(B, H, W, max(fg_channels, 3)), _out(B, H, W, 3) if want_bg else None
    rc = eng.lib.sdm_estimate_foreground(eng.h, _ptr(image), _ptr(alpha), B, H, W, 1e-5, 1.0, 10, 2, _ptr(fg), fg_channels, _ptr(bg), kind, None)
    return rc, (fg, bg) if want_bg else (fg,)


def _refine_alpha_guided(eng, kind, image, alpha, subsample=4):
    from comfyui_sdmatte_amd.engine import _ptr
    B, H, W, _ = image.shape
    out = _out(B, H, W)
    return eng.lib.sdm_refine_alpha_guided(eng.h, _ptr(image), _ptr(alpha), B, H, W, subsample, 2, 1e-4, _ptr(out), kind, None), (out,)


def _untouched(outs):
    return all(bool((o == SENTINEL).all()) for o in outs)


def _fresh(call, kind, *args, **kw):
    eng = _emu_engine()
    rc, outs = call(eng, kind, *args, **kw)
    eng.close()
    assert rc == 0 and not any(bool((o == SENTINEL).any()) for o in outs)
    return outs


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_emu_unknown_ptr_kind_is_invalid_weightless_calls(pkg):
    """ptr_kind = 2 at 8x8: SDM_ERR_INVALID with a message that names the argument, the outputs untouched, nothing allocated."""
    eng = _emu_engine()
    image, alpha = _rand(0, 1, 8, 8, 3), _rand(1, 1, 8, 8)
    for call, args in ((_make_trimap, (alpha,)), (_estimate_foreground, (image, alpha)), (_refine_alpha_guided, (image, alpha))):
        rc, outs = call(eng, 2, *args)
        assert rc == INVALID and b"ptr_kind" in eng.lib.sdm_last_error(eng.h), (call.__name__, rc)
        assert _untouched(outs), call.__name__
    assert eng.resident_bytes() == eng.weight_bytes()
    eng.close()


def test_emu_unknown_ptr_kind_is_invalid_model_calls(pkg):
    """ptr_kind = 2 on the tiny architecture at 64x64: sdm_forward_rect, sdm_apply_matte_node and sdm_apply_matte_mask return SDM_ERR_INVALID and
    leave alpha, matted and trimap untouched; the message names the argument, so nothing else about the call was at fault."""
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import _ptr
    from comfyui_sdmatte_amd.weights import synthetic_state_dict
    cfg = SDMatteConfig.tiny()
    eng = _emu_engine(cfg)
    eng.load_state_dict(synthetic_state_dict(cfg, 0))
    lib, h = eng.lib, eng.h
    nchw, aux = _rand(0, 1, 3, 64, 64) * 2 - 1, _rand(1, 1, 1, 64, 64) * 2 - 1
    image, tri = _rand(2, 1, 64, 64, 3), _rand(3, 1, 64, 64)

    a0, a1, a2, m1, m2, t2 = _out(1, 1, 64, 64), _out(1, 64, 64), _out(1, 64, 64), _out(1, 64, 64, 3), _out(1, 64, 64, 3), _out(1, 64, 64)
    before = eng.resident_bytes()
    for call, outs in (
            (lambda: lib.sdm_forward_rect(h, _ptr(nchw), _ptr(aux), 1, 64, 64, None, None, 4, 0, 1, _ptr(a0), 2, None), (a0,)),
            (lambda: lib.sdm_apply_matte_node(h, _ptr(image), _ptr(tri), 1, 64, 64, 64, 64, 64, 0, 0, 0, 0.8, _ptr(a1), _ptr(m1), 2, None), (a1, m1)),
            (lambda: lib.sdm_apply_matte_mask(h, _ptr(image), _ptr(tri), 1, 64, 64, 64, 64, 64, 0, 0.5, 1, 1, 0, 0, 0.8, _ptr(a2), _ptr(m2), _ptr(t2), 2,
                                              None), (a2, m2, t2))):
        lib.sdm_make_trimap(h, _ptr(tri), 1, 0, 64, 0.5, 0, 0, _ptr(t2), HOST, None)      # (another message in sdm_last_error)
        assert call() == INVALID and b"ptr_kind" in lib.sdm_last_error(h) and _untouched(outs)
    assert eng.resident_bytes() == before
    eng.close()


@pytest.mark.parametrize("kind", [HOST, DEVICE], ids=["host", "device"])
def test_emu_one_arena_across_call_kinds(pkg, kind):
    """make_trimap 40x50, estimate_foreground 97x131 (three large levels), refine_alpha_guided 70x67 at s = 4 and make_trimap again on ONE bare
    engine, whose arena and staging buffers each call finds as the previous one left them: every result is bit-equal to the same call on a fresh
    engine, resident_bytes never decreases, and release_memory gives everything but the weights back."""
    steps = ((_make_trimap, (_rand(0, 2, 40, 50),)),
             (_estimate_foreground, (_rand(1, 1, 97, 131, 3), _rand(2, 1, 97, 131))),
             (_refine_alpha_guided, (_rand(3, 1, 70, 67, 3), _rand(4, 1, 70, 67))),
             (_make_trimap, (_rand(0, 2, 40, 50),)))
    eng = _emu_engine()
    resident = [eng.resident_bytes()]
    assert resident[0] == eng.weight_bytes()
    for call, args in steps:
        rc, outs = call(eng, kind, *args)
        assert rc == 0, (call.__name__, eng.lib.sdm_last_error(eng.h))
        assert _same(outs, _fresh(call, kind, *args)), call.__name__
        resident.append(eng.resident_bytes())
    assert resident == sorted(resident) and resident[-1] > resident[0], resident
    eng.release_memory()
    assert eng.resident_bytes() == eng.weight_bytes()
    eng.close()


@pytest.mark.parametrize("kind", [HOST, DEVICE], ids=["host", "device"])
def test_emu_failed_call_leaves_no_state_behind(pkg, kind):
    """Between a good make_trimap and a good refine_alpha_guided: an estimate_foreground that fails its argument check (fg_channels = 5) and a
    refine_alpha_guided that fails in the scaffold (ptr_kind = 2).  The good call after them is bit-equal to a fresh engine's."""
    image, alpha = _rand(5, 1, 33, 47, 3), _rand(6, 1, 33, 47)
    eng = _emu_engine()
    assert _make_trimap(eng, kind, alpha)[0] == 0
    resident = eng.resident_bytes()
    rc, outs = _estimate_foreground(eng, kind, image, alpha, fg_channels=5)
    assert rc == INVALID and b"fg_channels" in eng.lib.sdm_last_error(eng.h) and _untouched(outs)
    rc, outs = _refine_alpha_guided(eng, 2, image, alpha)
    assert rc == INVALID and _untouched(outs)
    assert eng.resident_bytes() == resident
    rc, outs = _refine_alpha_guided(eng, kind, image, alpha)
    assert rc == 0 and _same(outs, _fresh(_refine_alpha_guided, kind, image, alpha))
    eng.close()
