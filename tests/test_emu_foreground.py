"""Foreground estimation on the kernel emulator: the two kernels of csrc/k_foreground.h (level arithmetic, nearest gathers, halos, tile seams, ragged
edges, the direct store of an all-small image) through sdm_estimate_foreground with host pointers, on an engine that never loaded weights.  The
real-kernel versions are tests/test_gpu_foreground.py."""
import ctypes
import os
import sys

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


def test_emu_estimate_foreground_case_list(emu):
    """Every case of the list against reference(fp64) under the suite's rule, and the launch counts of the whole run: one fg_small per call, one
    fg_level per large level."""
    import foreground_suite as FS
    emu.lib.kernel_counts(reset=True)
    FS.check(lambda im, a, p, rgba: emu.estimate_foreground(im, a, rgba=rgba, **p), lambda t: t)
    counts = emu.lib.kernel_counts()
    want_levels = sum(FS.n_large_levels(*c[1].shape[1:3]) for c in FS.cases())
    assert counts == {"fg_small": len(FS.cases()), "fg_level": want_levels}, counts


@pytest.mark.parametrize("H,W,levels", [(97, 131, 3), (5, 300, 4), (33, 70, 2), (150, 200, 3), (32, 32, 0), (1, 1, 0), (5, 20, 0), (1, 33, 1)])
def test_emu_estimate_foreground_launch_counts(emu, H, W, levels):
    """The launch count is part of the contract: fg_small = 1 and fg_level = the number of levels with max(h, w) > 32 - none for an all-small image."""
    import foreground_suite as FS
    assert FS.n_large_levels(H, W) == levels
    emu.lib.kernel_counts(reset=True)
    emu.estimate_foreground(torch.rand(2, H, W, 3), torch.rand(2, H, W))
    want = {"fg_small": 1}
    if levels:
        want["fg_level"] = levels
    assert emu.lib.kernel_counts() == want


def test_emu_estimate_foreground_batch_and_background_switch(emu):
    """B = 3 with different images: each image equals its own single-image result bit for bit (Jacobi steps: nothing depends on the batch position or
    the block order); want_background=False and rgba leave the foreground's bits alone."""
    import foreground_suite as FS
    image, alpha, _, _ = FS.scene(5, 3, 70, 67)
    image, alpha = torch.from_numpy(image), torch.from_numpy(alpha)
    assert not torch.equal(image[0], image[1]) and not torch.equal(alpha[1], alpha[2])
    fg, bg = emu.estimate_foreground(image, alpha)
    for b in range(3):
        f1, b1 = emu.estimate_foreground(image[b:b + 1], alpha[b:b + 1])
        assert torch.equal(fg[b:b + 1], f1) and torch.equal(bg[b:b + 1], b1)
    f2, none = emu.estimate_foreground(image, alpha, want_background=False)
    assert none is None and torch.equal(f2, fg)
    f4, b4 = emu.estimate_foreground(image, alpha, rgba=True)
    assert torch.equal(f4[..., :3], fg) and torch.equal(b4, bg) and torch.equal(f4[..., 3], alpha)
    small = torch.rand(2, 9, 30, 3), torch.rand(2, 9, 30)                # no large level: fg_small_kernel stores the outputs itself
    fs, bs = emu.estimate_foreground(*small)
    fn, _ = emu.estimate_foreground(*small, want_background=False)
    assert torch.equal(fs, fn) and torch.equal(emu.estimate_foreground(small[0][1:], small[1][1:])[1], bs[1:])


def test_emu_estimate_foreground_argument_checks_and_memory(emu):
    """Every parameter bound on both sides and a bad fg_channels: ValueError from Python, SDM_ERR_INVALID with a message from the C ABI; never
    SDM_ERR_STATE without weights; what the call keeps is counted by resident_bytes and given back by release_memory."""
    from comfyui_sdmatte_amd.engine import _ptr
    img, a = torch.rand(1, 40, 50, 3), torch.rand(1, 40, 50)
    good = {"regularization": 1e-5, "gradient_weight": 1.0, "n_small_iters": 10, "n_big_iters": 2}
    bad = ({"regularization": 0.0}, {"regularization": -1.0}, {"regularization": float("inf")}, {"gradient_weight": -1e-3}, {"gradient_weight": float("nan")},
           {"n_small_iters": 0}, {"n_small_iters": 65}, {"n_big_iters": 0}, {"n_big_iters": 5})
    for kw in bad:
        with pytest.raises(ValueError):
            emu.estimate_foreground(img, a, **kw)
    for kw in ({"regularization": 1e-9}, {"gradient_weight": 0.0}, {"n_small_iters": 1}, {"n_small_iters": 64}, {"n_big_iters": 1}, {"n_big_iters": 4}):
        emu.estimate_foreground(img, a, **kw)
    with pytest.raises(ValueError):
        emu.estimate_foreground(img[..., :2], a)
    with pytest.raises(ValueError):
        emu.estimate_foreground(img, a[:, :39])
    with pytest.raises(ValueError):
        emu.estimate_foreground(img[0], a[0])
    fg, bg = torch.empty(1, 40, 50, 4), torch.empty(1, 40, 50, 3)

    def raw(H=40, W=50, ch=3, **kw):
        p = dict(good, **kw)
        return emu.lib.sdm_estimate_foreground(emu.h, _ptr(img), _ptr(a), 1, H, W, p["regularization"], p["gradient_weight"], p["n_small_iters"],
                                               p["n_big_iters"], _ptr(fg), ch, _ptr(bg), 0, None)
    for kw in bad:
        assert raw(**kw) == -1 and next(iter(kw)).encode() in emu.lib.sdm_last_error(emu.h), kw
    for ch in (2, 5, 0):
        assert raw(ch=ch) == -1 and b"fg_channels" in emu.lib.sdm_last_error(emu.h)
    assert raw(H=0) == -1 and raw(W=0) == -1 and b"bad image size" in emu.lib.sdm_last_error(emu.h)
    assert raw(H=32769) == -1 and b"too large" in emu.lib.sdm_last_error(emu.h)
    assert raw() == 0 and raw(ch=4) == 0
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    emu.estimate_foreground(img, a)
    mid = emu.resident_bytes()
    assert mid >= emu.weight_bytes() + 20 * 25 * 32                      # arena: the plane of the small level (20, 25), 32 bytes per pixel
    assert raw() == 0                                                    # host pointers: image + alpha staged in, fg + bg staged out
    assert emu.resident_bytes() >= mid + 40 * 50 * 4 * (3 + 1 + 3 + 3)
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    emu.estimate_foreground(img, a)                                      # ... and the next call allocates again


def test_emu_fan_out_estimate_foreground(pkg):
    """MultiGpuEngine.estimate_foreground runs on the first engine and equals the single engine."""
    import foreground_suite as FS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.parallel import MultiGpuEngine
    one = _emu_engine()
    fan = MultiGpuEngine(SDMatteConfig.tiny(), [0, 1], _engine_factory=lambda d: _emu_engine())
    image, alpha, _, _ = FS.scene(9, 2, 41, 77)
    image, alpha = torch.from_numpy(image), torch.from_numpy(alpha)
    ff, fb = fan.estimate_foreground(image, alpha, 1e-4, 0.5, 4, 3, rgba=True)
    of, ob = one.estimate_foreground(image, alpha, 1e-4, 0.5, 4, 3, rgba=True)
    assert torch.equal(ff, of) and torch.equal(fb, ob)
    assert fan.estimate_foreground(image, alpha, want_background=False)[1] is None
    one.close(); fan.close()
