"""Motion-compensated temporal smoothing of the alpha on the kernel emulator: the kernel of csrc/k_motion.h (tile seams in both directions, halo lanes,
frame borders closer than `search`, both load paths, clips) through sdm_smooth_alpha_motion with host pointers, on an engine that never loaded weights.
The real-kernel versions are tests/test_gpu_motion.py."""
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


def _t(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in arrays)


def test_emu_smooth_motion_case_list(emu):
    """Every case of the list against reference(fp64) under the suite's rule, and the launch counts of the whole run: one per call."""
    import motion_suite as MS
    emu.lib.kernel_counts(reset=True)
    MS.check(lambda im, a, *p: emu.smooth_alpha_motion(im, a, *p), lambda t: t)
    assert emu.lib.kernel_counts() == {"tsm_smooth": len(MS.cases())}


def test_emu_smooth_motion_translation(emu):
    import motion_suite as MS
    MS.check_translation(lambda im, a, *p: emu.smooth_alpha_motion(im, a, *p), lambda t: t, "emulator")


def test_emu_smooth_motion_purpose(emu):
    import motion_suite as MS
    image, _, obs = MS.purpose_scene()
    MS.check_purpose(emu.smooth_alpha_motion(*_t(image, obs), *MS.PURPOSE).numpy(), "emulator")


@pytest.mark.parametrize("H,W,radius,patch", [(20, 70, 2, 1), (9, 72, 4, 2)])
def test_emu_smooth_motion_search_0_is_the_existing_call(emu, H, W, radius, patch):
    """search = 0: the launch and the bits of smooth_alpha_temporal; motion_penalty is not looked at."""
    import motion_suite as MS
    image, alpha = _t(*MS.inputs("dirty", 3, 5, H, W))
    emu.lib.kernel_counts(reset=True)
    out = emu.smooth_alpha_motion(image, alpha, radius, patch, 0, motion_penalty=0.3)
    assert emu.lib.kernel_counts() == {"ts_smooth": 1}
    assert torch.equal(out, emu.smooth_alpha_temporal(image, alpha, radius, patch))


@pytest.mark.parametrize("H,W,radius,patch,search,L", [(20, 70, 2, 1, 2, 2), (9, 72, 4, 2, 1, 3)])
def test_emu_smooth_motion_clips_equal_separate_calls(emu, H, W, radius, patch, search, L):
    """clip_len = L gives the bits of one call per clip (5 frames: the last clip is shorter); one launch either way."""
    import motion_suite as MS
    image, alpha = _t(*MS.inputs("dirty", 3, 5, H, W))
    emu.lib.kernel_counts(reset=True)
    out = emu.smooth_alpha_motion(image, alpha, radius, patch, search, clip_len=L)
    assert emu.lib.kernel_counts() == {"tsm_smooth": 1}
    for lo in range(0, 5, L):
        assert torch.equal(out[lo:lo + L], emu.smooth_alpha_motion(image[lo:lo + L], alpha[lo:lo + L], radius, patch, search)), lo
    assert not torch.equal(out, emu.smooth_alpha_motion(image, alpha, radius, patch, search))


@pytest.mark.parametrize("H,W,radius,patch,search", [(20, 70, 2, 1, 3), (9, 72, 4, 2, 2)])
def test_emu_smooth_motion_hard_cut_equals_its_shots(emu, H, W, radius, patch, search):
    """Every pixel of one shot differs from every pixel of the other by at least 0.4 per channel: every D across the cut is at least tau2 whatever the
    displacement, the weights there are exactly 0 and a zero weight is an exact no-op in both sums."""
    import motion_suite as MS
    image, alpha = _t(*MS.cut_scene(11, 3, 2, H, W))
    out = emu.smooth_alpha_motion(image, alpha, radius, patch, search)
    assert torch.equal(out[:3], emu.smooth_alpha_motion(image[:3], alpha[:3], radius, patch, search))
    assert torch.equal(out[3:], emu.smooth_alpha_motion(image[3:], alpha[3:], radius, patch, search))
    assert not torch.equal(out, torch.from_numpy(MS.sanitise_alpha(alpha.numpy())))


def test_emu_smooth_motion_identities(emu):
    """strength == 0, max_change == 0, B == 1, clip_len == 1 and 'every D of every candidate >= tau2' each return the sanitised alpha bit for bit."""
    import motion_suite as MS
    for H, W in ((20, 70), (9, 72)):
        image, alpha = _t(*MS.inputs("dirty", 5, 4, H, W))
        a = torch.from_numpy(MS.sanitise_alpha(alpha.numpy()))
        assert not torch.equal(emu.smooth_alpha_motion(image, alpha, search=2), a)
        assert torch.equal(emu.smooth_alpha_motion(image, alpha, search=2, strength=0.0), a)
        assert torch.equal(emu.smooth_alpha_motion(image, alpha, search=2, max_change=0.0), a)
        assert torch.equal(emu.smooth_alpha_motion(image, alpha, search=2, clip_len=1), a)
        assert torch.equal(emu.smooth_alpha_motion(image[:1], alpha[:1], 4, 2, 3), a[:1])
        # every frame differs from every other by at least 0.105 in every channel, at every pair of pixels: D >= 0.011 > tau2 = 0.01
        far = (0.125 * torch.arange(4).float().view(4, 1, 1, 1) + 0.02 * torch.rand(4, H, W, 3)).contiguous()
        assert torch.equal(emu.smooth_alpha_motion(far, alpha, 4, 2, 2, 0.1), a)


def test_emu_smooth_motion_load_paths_agree(emu):
    """Both load paths feed one arithmetic path: tensors that start 4 bytes off a 16-byte boundary (scalar path) give the bits of the aligned ones."""
    import motion_suite as MS
    for radius, patch, search, (H, W) in ((2, 1, 2, (20, 72)), (1, 2, 3, (9, 132)), (1, 0, 1, (15, 8))):
        image, alpha = _t(*MS.inputs("dirty", radius, 3, H, W))
        assert image.data_ptr() % 16 == 0 and alpha.data_ptr() % 16 == 0
        ref = emu.smooth_alpha_motion(image, alpha, radius, patch, search)
        assert torch.equal(ref, emu.smooth_alpha_motion(MS.offset_copy(image), MS.offset_copy(alpha), radius, patch, search)), (radius, patch)
        assert torch.equal(ref, emu.smooth_alpha_motion(image, MS.offset_copy(alpha), radius, patch, search)), (radius, patch)
        assert torch.equal(ref, emu.smooth_alpha_motion(image, alpha, radius, patch, search))


def test_emu_smooth_motion_argument_checks_and_memory(emu):
    """Every parameter bound on both sides: ValueError from Python, SDM_ERR_INVALID with the argument's name from the C ABI and nothing queued or written;
    never SDM_ERR_STATE without weights; what the call keeps is counted by resident_bytes and given back by release_memory."""
    from comfyui_sdmatte_amd.engine import Engine, _ptr
    assert Engine.TSM_MAX_SEARCH == 8
    img, a = torch.rand(3, 20, 24, 3), torch.rand(3, 20, 24)
    good = {"radius": 2, "patch": 1, "search": 2, "color_tolerance": 0.1, "motion_penalty": 0.02, "strength": 1.0, "max_change": 1.0, "clip_len": 0}
    nan, inf = float("nan"), float("inf")
    bad = ({"search": -1}, {"search": 9}, {"motion_penalty": -0.01}, {"motion_penalty": 1.0001}, {"motion_penalty": nan}, {"motion_penalty": inf},
           {"radius": 0}, {"radius": 5}, {"patch": -1}, {"patch": 3}, {"clip_len": -1}, {"clip_len": 4},
           {"color_tolerance": 0.0009}, {"color_tolerance": 1.0001}, {"color_tolerance": nan}, {"strength": -0.1}, {"strength": 1.0001}, {"strength": inf},
           {"max_change": -0.1}, {"max_change": 1.0001}, {"max_change": nan})
    for kw in bad:
        with pytest.raises(ValueError):
            emu.smooth_alpha_motion(img, a, **dict(good, **kw))
    for kw in ({"search": 1}, {"search": 8, "radius": 1}, {"motion_penalty": 0.0}, {"motion_penalty": 1.0}, {"clip_len": 1}, {"strength": 0.0}):
        emu.smooth_alpha_motion(img[:2, :8, :12].contiguous(), a[:2, :8, :12].contiguous(), **dict(good, **kw))
    with pytest.raises(ValueError):
        emu.smooth_alpha_motion(img[..., :2], a)
    with pytest.raises(ValueError):
        emu.smooth_alpha_motion(img, a[:, :19])
    with pytest.raises(ValueError):
        emu.smooth_alpha_motion(img, a, search=1.5)
    out = torch.full((3, 20, 24), -7.0)

    def raw(B=3, H=20, W=24, **kw):
        p = dict(good, **kw)
        return emu.lib.sdm_smooth_alpha_motion(emu.h, _ptr(img), _ptr(a), B, H, W, p["clip_len"], p["radius"], p["patch"], p["search"], p["color_tolerance"],
                                               p["motion_penalty"], p["strength"], p["max_change"], _ptr(out), 0, None)
    emu.lib.kernel_counts(reset=True)
    for kw in bad:
        assert raw(**kw) == -1 and next(iter(kw)).encode() in emu.lib.sdm_last_error(emu.h), kw
    assert raw(search=0, radius=5) == -1 and b"radius" in emu.lib.sdm_last_error(emu.h)
    assert raw(H=0) == -1 and raw(W=0) == -1 and raw(B=0) == -1 and b"bad image size" in emu.lib.sdm_last_error(emu.h)
    assert raw(H=32769) == -1 and b"too large" in emu.lib.sdm_last_error(emu.h)
    assert emu.lib.kernel_counts() == {} and bool((out == -7.0).all())      # nothing queued or written
    assert raw(search=0, motion_penalty=nan) == 0 and torch.equal(out, emu.smooth_alpha_temporal(img, a))      # (not looked at)
    assert raw() == 0 and torch.equal(out, emu.smooth_alpha_motion(img, a, search=2))
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    assert raw() == 0                                                    # host pointers: 3 + 1 floats per pixel staged in, 1 staged out
    assert emu.resident_bytes() >= emu.weight_bytes() + 3 * 20 * 24 * 4 * 5
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    emu.smooth_alpha_motion(img, a, search=1)                            # ... and the next call allocates again


def test_emu_fan_out_smooth_motion(pkg):
    """MultiGpuEngine.smooth_alpha_motion runs on the first engine and equals the single engine."""
    import motion_suite as MS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.parallel import MultiGpuEngine
    one = _emu_engine()
    fan = MultiGpuEngine(SDMatteConfig.tiny(), [0, 1], _engine_factory=lambda d: _emu_engine())
    image, alpha = _t(*MS.inputs("moving", 9, 4, 18, 66))
    assert torch.equal(fan.smooth_alpha_motion(image, alpha, 3, 2, 2, 0.05, 0.1, 0.5, 0.2, 3), one.smooth_alpha_motion(image, alpha, 3, 2, 2, 0.05, 0.1, 0.5, 0.2, 3))
    assert torch.equal(fan.smooth_alpha_motion(image, alpha, search=1), one.smooth_alpha_motion(image, alpha, 2, 1, 1, 0.1, 0.02, 1.0, 1.0, 0))
    one.close(); fan.close()
