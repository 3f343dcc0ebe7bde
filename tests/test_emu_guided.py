"""Guided alpha refinement on the kernel emulator: the kernels of csrc/k_guided.h (block means with ragged blocks, both load paths, window clipping,
tile seams and halos, the flat 4-pixel runs of the apply pass) through sdm_refine_alpha_guided with host pointers, on an engine that never loaded
weights.  The real-kernel versions are tests/test_gpu_guided.py."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

LAUNCHES = ("gf_mean", "gf_fit", "gf_smooth", "gf_apply")      # the four launches stated in csrc/k_guided.h


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


def test_emu_refine_alpha_case_list(emu):
    """Every case of the list against reference(fp64) under the suite's rule, and the launch counts of the whole run: four per call."""
    import guided_suite as GS
    emu.lib.kernel_counts(reset=True)
    GS.check(lambda im, a, s, r, eps: emu.refine_alpha_guided(im, a, s, r, eps), lambda t: t)
    assert emu.lib.kernel_counts() == {k: len(GS.cases()) for k in LAUNCHES}


@pytest.mark.parametrize("B,H,W,s,radius", [(1, 1, 1, 1, 1), (2, 70, 67, 4, 2), (3, 40, 64, 2, 32), (1, 200, 120, 16, 5), (1, 64, 64, 1, 24)])
def test_emu_refine_alpha_launch_counts(emu, B, H, W, s, radius):
    """The launch count is part of the contract: four, whatever B, H, W, subsample and radius."""
    emu.lib.kernel_counts(reset=True)
    emu.refine_alpha_guided(torch.rand(B, H, W, 3), torch.rand(B, H, W), s, radius)
    assert emu.lib.kernel_counts() == {k: 1 for k in LAUNCHES}


@pytest.mark.parametrize("H,W,s,radius", [(70, 67, 4, 2), (37, 64, 2, 3), (24, 40, 1, 9), (66, 48, 8, 1), (41, 77, 3, 32)])
def test_emu_refine_alpha_batch_equals_single_calls(emu, H, W, s, radius):
    """B = 3 with different images: each image equals its own single-image result bit for bit (direct sums in a fixed order; with H W no multiple of 4
    an image starts inside a 4-pixel run of the apply pass).  W = 64, 40, 48 take the 16-byte load path of the block means, the others the scalar one."""
    import guided_suite as GS
    image, alpha = GS._inputs("soft", 5, 3, H, W)
    image, alpha = torch.from_numpy(image), torch.from_numpy(alpha)
    assert not torch.equal(image[0], image[1]) and not torch.equal(alpha[1], alpha[2])
    out = emu.refine_alpha_guided(image, alpha, s, radius)
    for b in range(3):
        assert torch.equal(out[b:b + 1], emu.refine_alpha_guided(image[b:b + 1], alpha[b:b + 1], s, radius)), b


def test_emu_refine_alpha_load_paths_agree(emu):
    """The block means add in the same order with 16-byte loads and pixel by pixel: a tensor that starts 4 bytes off a 16-byte boundary (scalar path)
    gives the bits of the aligned one."""
    import guided_suite as GS
    for s in (1, 2, 4, 8):
        image, alpha = GS._inputs("dirty", s, 2, 40, 48)
        image, alpha = torch.from_numpy(image), torch.from_numpy(alpha)
        buf_i, buf_a = torch.empty(image.numel() + 1), torch.empty(alpha.numel() + 1)
        off_i, off_a = buf_i[1:].view(image.shape), buf_a[1:].view(alpha.shape)
        off_i.copy_(image); off_a.copy_(alpha)
        assert image.data_ptr() % 16 == 0 and off_i.data_ptr() % 16 == 4 and off_i.is_contiguous()
        assert torch.equal(emu.refine_alpha_guided(image, alpha, s), emu.refine_alpha_guided(off_i, off_a, s)), s


def test_emu_refine_alpha_argument_checks_and_memory(emu):
    """Every parameter bound on both sides: ValueError from Python, SDM_ERR_INVALID with a message from the C ABI; never SDM_ERR_STATE without
    weights; what the call keeps is counted by resident_bytes and given back by release_memory."""
    from comfyui_sdmatte_amd.engine import _ptr
    img, a = torch.rand(1, 40, 50, 3), torch.rand(1, 40, 50)
    good = {"subsample": 2, "radius": 2, "eps": 1e-4}
    bad = ({"subsample": 0}, {"subsample": 17}, {"subsample": -1}, {"radius": 0}, {"radius": 33}, {"eps": 0.0}, {"eps": 5e-7}, {"eps": 1.0001},
           {"eps": float("nan")}, {"eps": float("inf")}, {"eps": -1e-4})
    for kw in bad:
        with pytest.raises(ValueError):
            emu.refine_alpha_guided(img, a, **dict(good, **kw))
    for kw in ({"subsample": 1}, {"subsample": 16}, {"radius": 1}, {"radius": 32}, {"eps": 1e-6}, {"eps": 1.0}):
        emu.refine_alpha_guided(img, a, **dict(good, **kw))
    with pytest.raises(ValueError):
        emu.refine_alpha_guided(img[..., :2], a, 2)
    with pytest.raises(ValueError):
        emu.refine_alpha_guided(img, a[:, :39], 2)
    with pytest.raises(ValueError):
        emu.refine_alpha_guided(img[0], a[0], 2)
    out = torch.empty(1, 40, 50)

    def raw(H=40, W=50, **kw):
        p = dict(good, **kw)
        return emu.lib.sdm_refine_alpha_guided(emu.h, _ptr(img), _ptr(a), 1, H, W, p["subsample"], p["radius"], p["eps"], _ptr(out), 0, None)
    for kw in bad:
        assert raw(**kw) == -1 and next(iter(kw)).encode() in emu.lib.sdm_last_error(emu.h), kw
    assert raw(H=0) == -1 and raw(W=0) == -1 and b"bad image size" in emu.lib.sdm_last_error(emu.h)
    assert raw(H=32769) == -1 and b"too large" in emu.lib.sdm_last_error(emu.h)
    assert emu.lib.sdm_refine_alpha_guided(emu.h, _ptr(img), _ptr(a), 1 << 20, 1 << 10, 1 << 10, 2, 2, 1e-4, _ptr(out), 0, None) == -1
    assert b"too large" in emu.lib.sdm_last_error(emu.h)
    assert raw() == 0 and torch.equal(out, emu.refine_alpha_guided(img, a, 2))
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    emu.refine_alpha_guided(img, a, 2)
    mid = emu.resident_bytes()
    assert mid >= emu.weight_bytes() + 20 * 25 * 4 * 8                  # arena: the (a, b) and (abar, bbar) planes of the 20 x 25 grid at least
    assert raw() == 0                                                    # host pointers: 3 + 1 floats per pixel staged in, 1 staged out
    assert emu.resident_bytes() >= mid + 40 * 50 * 4 * 5
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    emu.refine_alpha_guided(img, a, 2)                                   # ... and the next call allocates again


def test_emu_fan_out_refine_alpha(pkg):
    """MultiGpuEngine.refine_alpha_guided runs on the first engine and equals the single engine."""
    import guided_suite as GS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.parallel import MultiGpuEngine
    one = _emu_engine()
    fan = MultiGpuEngine(SDMatteConfig.tiny(), [0, 1], _engine_factory=lambda d: _emu_engine())
    image, alpha = GS._inputs("soft", 9, 2, 41, 77)
    image, alpha = torch.from_numpy(image), torch.from_numpy(alpha)
    assert torch.equal(fan.refine_alpha_guided(image, alpha, 3, 4, 1e-3), one.refine_alpha_guided(image, alpha, 3, 4, 1e-3))
    assert torch.equal(fan.refine_alpha_guided(image, alpha, 2), one.refine_alpha_guided(image, alpha, 2, 2, 1e-4))
    one.close(); fan.close()
