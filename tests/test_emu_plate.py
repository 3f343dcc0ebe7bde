"""The clean plate on the kernel emulator: the three kernels of csrc/k_plate.h (missing children, the one-block kernel against the tiled ones, tile seams in
both directions, a fill that crosses a group of three fused levels, both load paths) through sdm_fill_background with host pointers, on an engine that
never loaded weights.  The real-kernel versions are tests/test_gpu_plate.py."""
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
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)) for a in arrays)


def test_emu_plate_case_list(emu):
    """Every case of the list against reference(fp64) under the suite's rule, and the launch counts of the whole run: the header's formula per case."""
    import plate_suite as PS
    emu.lib.kernel_counts(reset=True)
    PS.check(emu.fill_background, lambda t: t)
    assert emu.lib.kernel_counts() == PS.case_launches()


def test_emu_plate_launch_formula(emu):
    """1 + 2 ceil(S / 3) launches, S from H and W alone: per case size, in the bindings, and at most 8 at 2160 x 3840."""
    import plate_suite as PS
    for _, image, alpha, bg, hole, cut in PS.cases():
        H, W = image.shape[1:3]
        emu.lib.kernel_counts(reset=True)
        emu.fill_background(*_t(image, alpha, bg, hole), cut)
        want = PS.launches(H, W)
        assert emu.lib.kernel_counts() == want, (H, W)
        g = emu.plate_launches(H, W)
        assert g == (want.get("plate_pull", 0), 1, want.get("plate_push", 0)), (H, W)
    assert PS.levels_beyond_small(32, 32) == 0 and PS.levels_beyond_small(33, 31) == 1 and PS.levels_beyond_small(200, 300) == 4
    assert PS.levels_beyond_small(2160, 3840) == 7 and sum(PS.launches(2160, 3840).values()) == 7 <= 8
    assert sum(emu.plate_launches(2160, 3840)) == 7 and sum(emu.plate_launches(32768, 32768)) == 9


@pytest.mark.parametrize("H,W", [(67, 131), (40, 72), (20, 24)])
def test_emu_plate_identities(emu, H, W):
    """w_0 == 1 gives C; a channel that is 0 wherever w_0 > 0 stays 0; a flat background behind a hard alpha gives exactly 0.5: all bit for bit."""
    import plate_suite as PS
    assert (H, W) in PS.IDENTITY_SIZES
    PS.check_identities(emu.fill_background, lambda t: t, H, W, "emulator")


def test_emu_plate_flat_background_at_67x131(emu):
    """Identity 3 at the size the contract names, with a disc as the subject."""
    y, x = np.mgrid[0:67, 0:131]
    hard = (((y - 30) ** 2 + (x - 70) ** 2) <= 20 ** 2).astype(np.float32)[None]
    image = np.where(hard[..., None] == 0.0, np.float32(0.5), np.float32(0.9)).astype(np.float32) * np.ones((1, 67, 131, 3), np.float32)
    out = emu.fill_background(*_t(image, hard), alpha_cut=0.0625)
    assert bool((out == 0.5).all())


def test_emu_plate_serves_its_purpose(emu):
    import plate_suite as PS
    PS.check_purpose(emu.fill_background, lambda t: t, "emulator")


def test_emu_plate_all_subject_gives_zeros(emu):
    """An image with no pixel of w_0 > 0 gets an all-zero plate; its neighbour in the batch is filled as on its own."""
    import plate_suite as PS
    for H, W in ((20, 24), (70, 90)):
        image, alpha, _, _ = _t(*PS.inputs("soft", 5, 2, H, W))
        alpha[0] = 1.0
        out = emu.fill_background(image, alpha)
        assert bool((out[0] == 0.0).all()) and bool((out[1] != 0.0).any())
        assert torch.equal(out[1:], emu.fill_background(image[1:].contiguous(), alpha[1:].contiguous()))
        alpha[0] = 0.0625                                               # a >= alpha_cut everywhere is all subject too
        assert bool((emu.fill_background(image, alpha)[0] == 0.0).all())


@pytest.mark.parametrize("H,W", [(67, 131), (40, 72), (20, 24)])
def test_emu_plate_batch_equals_single_calls(emu, H, W):
    import plate_suite as PS
    image, alpha, bg, hole = _t(*PS.inputs("dirty", 7, 3, H, W, with_bg=True, with_hole=True))
    out = emu.fill_background(image, alpha, bg, hole, 0.25)
    assert torch.equal(out, emu.fill_background(image, alpha, bg, hole, 0.25))
    for b in range(3):
        assert torch.equal(out[b:b + 1], emu.fill_background(*(t[b:b + 1].contiguous() for t in (image, alpha, bg, hole)), 0.25)), b


def test_emu_plate_load_paths_agree(emu):
    """Both load paths feed one arithmetic path: tensors that start 4 bytes off a 16-byte boundary (scalar path) give the bits of the aligned ones."""
    import plate_suite as PS
    for H, W in ((40, 72), (33, 136), (20, 24)):
        image, alpha, bg, hole = _t(*PS.inputs("dirty", H, 2, H, W, with_bg=True, with_hole=True))
        assert all(t.data_ptr() % 16 == 0 for t in (image, alpha, bg, hole))
        ref = emu.fill_background(image, alpha, bg, hole, 0.25)
        off = [PS.offset_copy(t) for t in (image, alpha, bg, hole)]
        assert torch.equal(ref, emu.fill_background(*off, 0.25)), (H, W)
        assert torch.equal(ref, emu.fill_background(image, off[1], bg, hole, 0.25)), (H, W)
        assert torch.equal(ref, emu.fill_background(image, alpha, bg, off[3], 0.25)), (H, W)
        assert torch.equal(emu.fill_background(image, alpha), emu.fill_background(off[0], off[1])), (H, W)


def test_emu_plate_argument_checks_and_memory(emu):
    """Every parameter bound on both sides: ValueError from Python, SDM_ERR_INVALID with the argument's name from the C ABI and nothing queued or written;
    never SDM_ERR_STATE without weights; what the call keeps is counted by resident_bytes and given back by release_memory."""
    import plate_suite as PS
    from comfyui_sdmatte_amd.engine import _ptr
    img, a = torch.rand(2, 40, 72, 3), torch.rand(2, 40, 72)
    nan, inf = float("nan"), float("inf")
    bad = (2.0 ** -11, 0.0, -0.5, 1.0001, nan, inf)
    for cut in bad:
        with pytest.raises(ValueError):
            emu.fill_background(img, a, alpha_cut=cut)
    with pytest.raises(ValueError):
        emu.fill_background(img, a, alpha_cut="0.5")
    for cut in (2.0 ** -10, 1.0):
        emu.fill_background(img[:1, :8, :12].contiguous(), a[:1, :8, :12].contiguous(), alpha_cut=cut)
    for args in ((img[..., :2], a), (img, a[:, :19]), (img[0], a[0])):
        with pytest.raises(ValueError):
            emu.fill_background(*args)
    with pytest.raises(ValueError):
        emu.fill_background(img, a, bg=img[:1])
    with pytest.raises(ValueError):
        emu.fill_background(img, a, hole=a[:, :5])
    out = torch.full((2, 40, 72, 3), -7.0)

    def raw(B=2, H=40, W=72, cut=0.0625):
        return emu.lib.sdm_fill_background(emu.h, _ptr(img), _ptr(a), None, None, B, H, W, cut, _ptr(out), 0, None)
    emu.lib.kernel_counts(reset=True)
    for cut in bad:
        assert raw(cut=cut) == -1 and b"alpha_cut" in emu.lib.sdm_last_error(emu.h), cut
    assert raw(H=0) == -1 and raw(W=0) == -1 and raw(B=0) == -1 and b"bad image size" in emu.lib.sdm_last_error(emu.h)
    assert raw(H=32769) == -1 and b"too large" in emu.lib.sdm_last_error(emu.h)
    assert emu.lib.kernel_counts() == {} and bool((out == -7.0).all())      # nothing queued or written
    assert raw() == 0 and torch.equal(out, emu.fill_background(img, a))
    assert emu.lib.kernel_counts() == PS.launches(40, 72, calls=2)
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    assert raw() == 0                      # host pointers: 3 + 1 floats per pixel staged in, 3 staged out, and level 1 of the pyramid (4 floats per 4 pixels)
    assert emu.resident_bytes() >= emu.weight_bytes() + 2 * 40 * 72 * 4 * (4 + 3 + 1)
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    emu.fill_background(img, a, alpha_cut=1.0)                              # ... and the next call allocates again
