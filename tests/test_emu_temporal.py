"""Temporal smoothing of the alpha on the kernel emulator: the kernel of csrc/k_temporal.h (ring start and wrap, ragged tiles, tile seams and halos, both
load paths, clips) through sdm_smooth_alpha_temporal with host pointers, on an engine that never loaded weights.  The real-kernel versions are
tests/test_gpu_temporal.py."""
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


def test_emu_smooth_alpha_case_list(emu):
    """Every case of the list against reference(fp64) under the suite's rule, and the launch counts of the whole run: one per call."""
    import temporal_suite as TS
    emu.lib.kernel_counts(reset=True)
    TS.check(lambda im, a, *p: emu.smooth_alpha_temporal(im, a, *p), lambda t: t)
    assert emu.lib.kernel_counts() == {"ts_smooth": len(TS.cases())}


def test_emu_smooth_alpha_purpose(emu):
    import temporal_suite as TS
    image, _, obs = TS.purpose_scene()
    TS.check_purpose(emu.smooth_alpha_temporal(*_t(image, obs), *TS.PURPOSE).numpy(), "emulator")


@pytest.mark.parametrize("H,W,radius,patch,L", [(33, 70, 2, 1, 3), (20, 72, 4, 2, 5), (9, 130, 1, 0, 2), (15, 8, 3, 1, 4)])
def test_emu_smooth_alpha_clips_equal_separate_calls(emu, H, W, radius, patch, L):
    """clip_len = L gives the bits of one call per clip (11 frames: the last clip is shorter); one launch either way."""
    import temporal_suite as TS
    image, alpha = _t(*TS._inputs("dirty", 3, 11, H, W))
    emu.lib.kernel_counts(reset=True)
    out = emu.smooth_alpha_temporal(image, alpha, radius, patch, clip_len=L)
    assert emu.lib.kernel_counts() == {"ts_smooth": 1}
    for lo in range(0, 11, L):
        assert torch.equal(out[lo:lo + L], emu.smooth_alpha_temporal(image[lo:lo + L], alpha[lo:lo + L], radius, patch)), lo
    assert not torch.equal(out, emu.smooth_alpha_temporal(image, alpha, radius, patch))


@pytest.mark.parametrize("H,W,radius,patch", [(33, 70, 2, 1), (20, 72, 4, 2), (9, 132, 1, 0)])
def test_emu_smooth_alpha_hard_cut_equals_its_shots(emu, H, W, radius, patch):
    """Every D across the cut is at least tau2: the weights there are exactly 0 and a zero weight is an exact no-op in both sums."""
    import temporal_suite as TS
    image, alpha = _t(*TS.cut_scene(11, 5, 4, H, W))
    out = emu.smooth_alpha_temporal(image, alpha, radius, patch)
    assert torch.equal(out[:5], emu.smooth_alpha_temporal(image[:5], alpha[:5], radius, patch))
    assert torch.equal(out[5:], emu.smooth_alpha_temporal(image[5:], alpha[5:], radius, patch))
    assert not torch.equal(out, torch.from_numpy(TS.sanitise_alpha(alpha.numpy())))


def test_emu_smooth_alpha_identities(emu):
    """strength == 0, max_change == 0, B == 1, clip_len == 1 and 'every D >= tau2' each return the sanitised alpha bit for bit."""
    import temporal_suite as TS
    for H, W in ((33, 70), (9, 72)):
        image, alpha = _t(*TS._inputs("dirty", 5, 6, H, W))
        a = torch.from_numpy(TS.sanitise_alpha(alpha.numpy()))
        assert not torch.equal(emu.smooth_alpha_temporal(image, alpha), a)
        assert torch.equal(emu.smooth_alpha_temporal(image, alpha, strength=0.0), a)
        assert torch.equal(emu.smooth_alpha_temporal(image, alpha, max_change=0.0), a)
        assert torch.equal(emu.smooth_alpha_temporal(image, alpha, clip_len=1), a)
        assert torch.equal(emu.smooth_alpha_temporal(image[:1], alpha[:1], 4, 2), a[:1])
        # every frame differs from every other by at least 0.1 in every channel: D >= 0.01 = tau2 at color_tolerance 0.1 ... (0.125 keeps it clear of rounding)
        far = (0.125 * torch.arange(6).float().view(6, 1, 1, 1) + 0.02 * torch.rand(1, H, W, 3)).expand(6, H, W, 3).contiguous()
        assert torch.equal(emu.smooth_alpha_temporal(far, alpha, 4, 2, 0.1), a)


def test_emu_smooth_alpha_load_paths_agree(emu):
    """Both load paths add in the same order: tensors that start 4 bytes off a 16-byte boundary (scalar path) give the bits of the aligned ones."""
    import temporal_suite as TS
    for radius, patch, (H, W) in ((2, 1, (20, 72)), (4, 2, (9, 132)), (1, 0, (15, 8))):
        image, alpha = _t(*TS._inputs("dirty", radius, 6, H, W))
        assert image.data_ptr() % 16 == 0 and alpha.data_ptr() % 16 == 0
        ref = emu.smooth_alpha_temporal(image, alpha, radius, patch)
        assert torch.equal(ref, emu.smooth_alpha_temporal(TS.offset_copy(image), TS.offset_copy(alpha), radius, patch)), (radius, patch)
        assert torch.equal(ref, emu.smooth_alpha_temporal(image, TS.offset_copy(alpha), radius, patch)), (radius, patch)
        assert torch.equal(ref, emu.smooth_alpha_temporal(image, alpha, radius, patch))


def test_emu_smooth_alpha_argument_checks_and_memory(emu):
    """Every parameter bound on both sides: ValueError from Python, SDM_ERR_INVALID with the argument's name from the C ABI; never SDM_ERR_STATE without
    weights; what the call keeps is counted by resident_bytes and given back by release_memory."""
    from comfyui_sdmatte_amd.engine import Engine, _ptr
    assert (Engine.TS_MAX_RADIUS, Engine.TS_MAX_PATCH) == (4, 2)
    img, a = torch.rand(3, 20, 24, 3), torch.rand(3, 20, 24)
    good = {"radius": 2, "patch": 1, "color_tolerance": 0.1, "strength": 1.0, "max_change": 1.0, "clip_len": 0}
    nan, inf = float("nan"), float("inf")
    bad = ({"radius": 0}, {"radius": 5}, {"radius": -1}, {"patch": -1}, {"patch": 3}, {"clip_len": -1}, {"clip_len": 4},
           {"color_tolerance": 0.0}, {"color_tolerance": 0.0009}, {"color_tolerance": 1.0001}, {"color_tolerance": nan}, {"color_tolerance": inf},
           {"strength": -0.1}, {"strength": 1.0001}, {"strength": nan}, {"strength": inf},
           {"max_change": -0.1}, {"max_change": 1.0001}, {"max_change": nan}, {"max_change": inf})
    for kw in bad:
        with pytest.raises(ValueError):
            emu.smooth_alpha_temporal(img, a, **dict(good, **kw))
    for kw in ({"radius": 1}, {"radius": 4}, {"patch": 0}, {"patch": 2}, {"clip_len": 3}, {"clip_len": 1}, {"color_tolerance": 1.0 / 1024.0},
               {"color_tolerance": 1.0}, {"strength": 0.0}, {"max_change": 0.0}):
        emu.smooth_alpha_temporal(img, a, **dict(good, **kw))
    with pytest.raises(ValueError):
        emu.smooth_alpha_temporal(img[..., :2], a)
    with pytest.raises(ValueError):
        emu.smooth_alpha_temporal(img, a[:, :19])
    with pytest.raises(ValueError):
        emu.smooth_alpha_temporal(img[0], a[0])
    with pytest.raises(ValueError):
        emu.smooth_alpha_temporal(img, a, radius=1.5)
    out = torch.full((3, 20, 24), -7.0)

    def raw(B=3, H=20, W=24, **kw):
        p = dict(good, **kw)
        return emu.lib.sdm_smooth_alpha_temporal(emu.h, _ptr(img), _ptr(a), B, H, W, p["clip_len"], p["radius"], p["patch"], p["color_tolerance"],
                                                 p["strength"], p["max_change"], _ptr(out), 0, None)
    emu.lib.kernel_counts(reset=True)
    for kw in bad:
        assert raw(**kw) == -1 and next(iter(kw)).encode() in emu.lib.sdm_last_error(emu.h), kw
    assert raw(H=0) == -1 and raw(W=0) == -1 and raw(B=0) == -1 and b"bad image size" in emu.lib.sdm_last_error(emu.h)
    assert raw(H=32769) == -1 and b"too large" in emu.lib.sdm_last_error(emu.h)
    assert raw(B=1 << 20, H=1 << 10, W=1 << 10) == -1 and b"too large" in emu.lib.sdm_last_error(emu.h)
    assert emu.lib.kernel_counts() == {} and bool((out == -7.0).all())      # nothing queued or written
    assert raw() == 0 and torch.equal(out, emu.smooth_alpha_temporal(img, a))
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    assert raw() == 0                                                    # host pointers: 3 + 1 floats per pixel staged in, 1 staged out
    assert emu.resident_bytes() >= emu.weight_bytes() + 3 * 20 * 24 * 4 * 5
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    emu.smooth_alpha_temporal(img, a)                                    # ... and the next call allocates again


def test_emu_fan_out_smooth_alpha(pkg):
    """MultiGpuEngine.smooth_alpha_temporal runs on the first engine and equals the single engine."""
    import temporal_suite as TS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.parallel import MultiGpuEngine
    one = _emu_engine()
    fan = MultiGpuEngine(SDMatteConfig.tiny(), [0, 1], _engine_factory=lambda d: _emu_engine())
    image, alpha = _t(*TS._inputs("moving", 9, 7, 21, 77))
    assert torch.equal(fan.smooth_alpha_temporal(image, alpha, 4, 2, 0.05, 0.5, 0.2, 3), one.smooth_alpha_temporal(image, alpha, 4, 2, 0.05, 0.5, 0.2, 3))
    assert torch.equal(fan.smooth_alpha_temporal(image, alpha), one.smooth_alpha_temporal(image, alpha, 2, 1, 0.1, 1.0, 1.0, 0))
    one.close(); fan.close()
