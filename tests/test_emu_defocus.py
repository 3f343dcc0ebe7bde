"""Background defocus on the kernel emulator: the two kernels of csrc/k_defocus.h (segment boundaries, tile seams in both directions, borders closer than
the radius, both load paths) through sdm_defocus_background with host pointers, on an engine that never loaded weights.  The real-kernel versions are
tests/test_gpu_defocus.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

LAUNCHES = ("dof_prefix", "dof_gather")      # include/sdmatte.h: two launches per call, whatever the arguments


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


def _t(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)) for a in arrays)


def test_emu_defocus_case_list(emu):
    """Every case of the list against reference(fp64) under the suite's rule, and the launch counts of the whole run: two per call."""
    import defocus_suite as DS
    emu.lib.kernel_counts(reset=True)
    DS.check(emu.defocus_background, lambda t: t)
    assert emu.lib.kernel_counts() == {k: len(DS.cases()) for k in LAUNCHES}


def test_emu_defocus_purpose_and_disc_shape(emu):
    import defocus_suite as DS
    image, alpha = _t(*DS.purpose_scene())
    DS.check_purpose(emu.defocus_background(image, alpha, None, None, DS.PURPOSE_R, 0.0, 0.5).numpy(), "emulator")
    DS.check_disc_shape(emu.defocus_background, lambda t: t, "emulator")


@pytest.mark.parametrize("H,W,R", [(40, 70, 5), (9, 260, 17)])
def test_emu_defocus_identities(emu, H, W, R):
    """a == 1 gives F; a channel with w C == 0 everywhere gives a F; a batch of 2 equals two calls: all bit for bit."""
    import defocus_suite as DS
    image, alpha, fg, bg = _t(*DS.inputs("dirty", 3, 2, H, W, planes=True))
    a = torch.from_numpy(DS.sanitise_alpha(alpha.numpy()))
    assert bool((a == 1.0).any()) and bool((a < 1.0).any())
    out = emu.defocus_background(image, alpha, fg, bg, R, 4.0, 0.5)
    assert torch.equal(out[a == 1.0], fg[a == 1.0]) and not torch.equal(out, fg)
    assert torch.equal(emu.defocus_background(image, alpha, None, None, R)[a == 1.0], image[a == 1.0])
    bg0 = bg.clone(); bg0[..., 1] = 0.0
    assert torch.equal(emu.defocus_background(image, alpha, fg, bg0, R, 4.0, 0.5)[..., 1], a * fg[..., 1])
    for b in range(2):
        assert torch.equal(out[b:b + 1], emu.defocus_background(image[b:b + 1], alpha[b:b + 1], fg[b:b + 1], bg[b:b + 1], R, 4.0, 0.5)), b
    assert torch.equal(out, emu.defocus_background(image, alpha, fg, bg, R, 4.0, 0.5))


def test_emu_defocus_subject_larger_than_the_disc(emu):
    """Deep inside a hard subject every weight of the disc is 0: N = 0, the floor keeps the division finite and out is F there, bit for bit."""
    import defocus_suite as DS
    image, alpha, fg, bg = _t(*DS.inputs("hard", 1, 1, 70, 130, planes=True))
    assert bool((alpha[0, 25:45, 50:80] == 1.0).all())
    out = emu.defocus_background(image, alpha, fg, bg, 5, 4.0, 0.5)
    assert bool(torch.isfinite(out).all()) and torch.equal(out[alpha == 1.0], fg[alpha == 1.0])


def test_emu_defocus_load_paths_agree(emu):
    """Both load paths feed one arithmetic path: tensors that start 4 bytes off a 16-byte boundary (scalar path) give the bits of the aligned ones."""
    import defocus_suite as DS
    for R, (H, W) in ((2, (20, 72)), (17, (9, 264)), (5, (15, 8))):
        image, alpha, fg, bg = _t(*DS.inputs("dirty", R, 2, H, W, planes=True))
        assert image.data_ptr() % 16 == 0 and alpha.data_ptr() % 16 == 0 and bg.data_ptr() % 16 == 0
        ref = emu.defocus_background(image, alpha, fg, bg, R, 4.0, 0.5)
        off = [DS.offset_copy(t) for t in (image, alpha, fg, bg)]
        assert torch.equal(ref, emu.defocus_background(*off, R, 4.0, 0.5)), R
        assert torch.equal(ref, emu.defocus_background(image, off[1], fg, bg, R, 4.0, 0.5)), R
        assert torch.equal(emu.defocus_background(image, alpha, None, None, R), emu.defocus_background(off[0], off[1], None, None, R)), R


def test_emu_defocus_argument_checks_and_memory(emu):
    """Every parameter bound on both sides: ValueError from Python, SDM_ERR_INVALID with the argument's name from the C ABI and nothing queued or written;
    never SDM_ERR_STATE without weights; what the call keeps is counted by resident_bytes and given back by release_memory."""
    from comfyui_sdmatte_amd.engine import _ptr
    img, a = torch.rand(2, 20, 24, 3), torch.rand(2, 20, 24)
    good = {"radius_px": 3, "highlight_gain": 1.0, "highlight_threshold": 0.5}
    nan, inf = float("nan"), float("inf")
    bad = ({"radius_px": 0}, {"radius_px": -1}, {"radius_px": 65}, {"highlight_gain": -0.01}, {"highlight_gain": 64.5}, {"highlight_gain": nan},
           {"highlight_gain": inf}, {"highlight_threshold": -0.01}, {"highlight_threshold": 1.0001}, {"highlight_threshold": nan})
    for kw in bad:
        with pytest.raises(ValueError):
            emu.defocus_background(img, a, **dict(good, **kw))
    for kw in ({"radius_px": 1}, {"radius_px": 64}, {"highlight_gain": 0.0}, {"highlight_gain": 64.0}, {"highlight_threshold": 0.0}, {"highlight_threshold": 1.0}):
        emu.defocus_background(img[:1, :8, :12].contiguous(), a[:1, :8, :12].contiguous(), **dict(good, **kw))
    with pytest.raises(ValueError):
        emu.defocus_background(img[..., :2], a)
    with pytest.raises(ValueError):
        emu.defocus_background(img, a[:, :19])
    with pytest.raises(ValueError):
        emu.defocus_background(img, a, fg=img[:1])
    with pytest.raises(ValueError):
        emu.defocus_background(img, a, radius_px=1.5)
    out = torch.full((2, 20, 24, 3), -7.0)

    def raw(B=2, H=20, W=24, **kw):
        p = dict(good, **kw)
        return emu.lib.sdm_defocus_background(emu.h, _ptr(img), _ptr(a), None, None, B, H, W, p["radius_px"], p["highlight_gain"], p["highlight_threshold"],
                                              _ptr(out), 0, None)
    emu.lib.kernel_counts(reset=True)
    for kw in bad:
        assert raw(**kw) == -1 and next(iter(kw)).encode() in emu.lib.sdm_last_error(emu.h), kw
    assert raw(H=0) == -1 and raw(W=0) == -1 and raw(B=0) == -1 and b"bad image size" in emu.lib.sdm_last_error(emu.h)
    assert raw(H=32769) == -1 and b"too large" in emu.lib.sdm_last_error(emu.h)
    assert emu.lib.kernel_counts() == {} and bool((out == -7.0).all())      # nothing queued or written
    assert raw() == 0 and torch.equal(out, emu.defocus_background(img, a, **good))
    assert emu.lib.kernel_counts() == {k: 2 for k in LAUNCHES}
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    assert raw() == 0                      # host pointers: 3 + 1 floats per pixel staged in, 3 staged out, and the prefix plane of 4 in the arena
    assert emu.resident_bytes() >= emu.weight_bytes() + 2 * 20 * 24 * 4 * (4 + 3 + 4)
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    emu.defocus_background(img, a, radius_px=1)                             # ... and the next call allocates again
