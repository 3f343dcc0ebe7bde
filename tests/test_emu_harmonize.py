"""Harmonize on the kernel emulator: the four kernels of csrc/k_harmonize.h (ragged runs, segment and tile seams, borders closer than the wrap radius, both
load paths, every stage on and off) through sdm_harmonize with host pointers, on an engine that never loaded weights.  The real-kernel versions are
tests/test_gpu_harmonize.py."""
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


def _full(eng):
    return lambda *p, **kw: eng.harmonize(*p, return_fg=True, return_map=True, **kw)


def test_emu_harmonize_case_list_and_launch_counts(emu):
    """Every case of the list against reference(fp64) under the suite's rule, and the launch counts of the whole run: per case the stages that are on."""
    import harmonize_suite as HS
    emu.lib.kernel_counts(reset=True)
    HS.check(_full(emu), lambda t: t)
    assert emu.lib.kernel_counts() == HS.expected_counts([c[4] for c in HS.cases()])


@pytest.mark.parametrize("params,want", [((0.6, 0.8, 0.5, 0.5, 6.0), ("hz_stats", "hz_finalize", "hz_rows", "hz_compose")),
                                         ((0.6, 0.0, 0.5, 0.0, 6.0), ("hz_stats", "hz_finalize", "hz_compose")),
                                         ((0.0, 0.3, 0.0, 0.0, 99.0), ("hz_stats", "hz_finalize", "hz_compose")),
                                         ((0.0, 0.0, 1.0, 0.2, 0.3), ("hz_rows", "hz_compose")), ((0.0, 0.0, 1.0, 0.0, -1.0), ("hz_compose", ))])
def test_emu_harmonize_launches_per_stage_combination(emu, params, want):
    """4 launches with everything on, 3 without the wrap, 2 without the match, 1 with neither, whatever the size; without the wrap the sigma is not looked
    at; without the match the map is the identity, and it is written all the same."""
    import harmonize_suite as HS
    assert HS.stages_on(params) == want
    for H, W in ((9, 37), (67, 130)):
        fg, alpha, bg = _t(*HS.inputs("soft", 1, 2, H, W))
        emu.lib.kernel_counts(reset=True)
        _, _, m = _full(emu)(fg, alpha, bg, *params)
        assert emu.lib.kernel_counts() == {k: 1 for k in want}
        if "hz_stats" not in want:
            assert torch.equal(m, torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]).repeat(2, 1))


def test_emu_harmonize_exact_statistics(emu):
    import harmonize_suite as HS
    fg, alpha, bg, params, _, _ = HS.exact_case()
    HS.check_exact(emu.harmonize(*_t(fg, alpha, bg), *params, return_map=True)[1].numpy(), "emulator")


def test_emu_harmonize_purpose_scenes(emu):
    import harmonize_suite as HS
    fg, alpha, bg, params = HS.match_scene()
    HS.check_match_purpose(emu.harmonize(*_t(fg, alpha, bg), *params, return_fg=True)[1].numpy(), "emulator")
    fg, alpha, bg, params = HS.wrap_scene()
    HS.check_wrap_purpose(emu.harmonize(*_t(fg, alpha, bg), *params, return_fg=True)[1].numpy(), "emulator")


@pytest.mark.parametrize("H,W,sigma", [(40, 70, 2.0), (9, 260, 6.0)])
def test_emu_harmonize_identities(emu, H, W, sigma):
    """The six identities of the header, bit for bit."""
    import harmonize_suite as HS
    fg, alpha, bg = _t(*HS.inputs("dirty", 3, 2, H, W))
    a = torch.from_numpy(HS.sanitise_alpha(alpha.numpy()))
    assert bool((a == 1.0).any()) and bool((a == 0.0).any())
    params = (0.6, 0.8, 0.5, 0.5, sigma)
    out, fgo, m = _full(emu)(fg, alpha, bg, *params)
    assert torch.equal(out[a == 0.0], bg[a == 0.0])                                                    # 1
    assert torch.equal(out[a == 1.0], fgo[a == 1.0]) and not torch.equal(out, fgo)                     # 2
    out0, fgo0, _ = _full(emu)(fg, alpha, bg, 0.0, 0.0, 0.0, 0.0, sigma)                               # 3
    assert torch.equal(fgo0, fg) and torch.equal(out0, a.unsqueeze(-1) * fg + (1.0 - a).unsqueeze(-1) * bg)
    for b in range(2):                                                                                 # 5: batch against per-image calls
        one = _full(emu)(fg[b:b + 1], alpha[b:b + 1], bg[b:b + 1], *params)
        assert all(torch.equal(x[b:b + 1], y) for x, y in zip((out, fgo, m), one)), b
    again = _full(emu)(fg, alpha, bg, *params)
    assert all(torch.equal(x, y) for x, y in zip((out, fgo, m), again))
    rep = _full(emu)(fg, alpha, bg[:1].repeat(2, 1, 1, 1), *params)                                    # 6
    single = _full(emu)(fg, alpha, bg[:1].contiguous(), *params)
    assert all(torch.equal(x, y) for x, y in zip(rep, single))


def test_emu_harmonize_wrap_leaves_the_deep_interior_alone(emu):
    """Identity 4: where every existing pixel within Chebyshev distance r has a == 1, fg_out equals that of the same call without the wrap; elsewhere the
    wrap did something."""
    import harmonize_suite as HS
    fg, alpha, bg = _t(*HS.inputs("hard", 1, 1, 70, 130))
    sigma = 2.0
    r = HS.wrap_weights(sigma)[0]
    a = alpha[0].numpy()
    deep = np.zeros_like(a, bool)
    for y in range(a.shape[0]):
        for x in range(a.shape[1]):
            deep[y, x] = bool((a[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] == 1.0).all())
    assert deep.sum() > 100 and (~deep).sum() > 100
    with_wrap = emu.harmonize(fg, alpha, bg, 0.6, 0.8, 0.5, 0.7, sigma, return_fg=True)[1][0].numpy()
    without = emu.harmonize(fg, alpha, bg, 0.6, 0.8, 0.5, 0.0, sigma, return_fg=True)[1][0].numpy()
    assert np.array_equal(with_wrap[deep], without[deep]) and not np.array_equal(with_wrap[~deep], without[~deep])


def test_emu_harmonize_load_paths_agree(emu):
    """Both load paths feed one arithmetic path: tensors that start 4 bytes off a 16-byte boundary (scalar path) give the bits of the aligned ones."""
    import harmonize_suite as HS
    for sigma, (H, W) in ((0.5, (20, 72)), (6.0, (9, 264)), (2.0, (15, 8))):
        fg, alpha, bg = _t(*HS.inputs("dirty", int(sigma), 2, H, W))
        assert all(t.data_ptr() % 16 == 0 for t in (fg, alpha, bg))
        params = (0.6, 0.8, 0.5, 0.5, sigma)
        ref = _full(emu)(fg, alpha, bg, *params)
        off = [HS.offset_copy(t) for t in (fg, alpha, bg)]
        for variant in (off, (fg, off[1], bg), (off[0], alpha, off[2])):
            assert all(torch.equal(x, y) for x, y in zip(ref, _full(emu)(*variant, *params))), sigma


def test_emu_harmonize_argument_checks_and_memory(emu):
    """Every limit on both sides: ValueError from Python, SDM_ERR_INVALID with the argument's name from the C ABI and nothing queued or written; never
    SDM_ERR_STATE without weights; what the call keeps is counted by resident_bytes and given back by release_memory."""
    from comfyui_sdmatte_amd.engine import _ptr
    fg, a, bg = torch.rand(2, 20, 24, 3), torch.rand(2, 20, 24), torch.rand(2, 20, 24, 3)
    good = {"luma_strength": 0.5, "chroma_strength": 0.5, "contrast_strength": 0.5, "wrap_strength": 0.5, "wrap_sigma": 2.0}
    nan, inf = float("nan"), float("inf")
    bad = [{k: v} for k in ("luma_strength", "chroma_strength", "contrast_strength", "wrap_strength") for v in (-0.01, 1.01, nan, inf)]
    bad += [{"wrap_sigma": v} for v in (0.0, -1.0, 16.5, nan, inf)]
    for kw in bad:
        with pytest.raises(ValueError):
            emu.harmonize(fg, a, bg, **dict(good, **kw))
    for kw in ({"luma_strength": 0.0}, {"luma_strength": 1.0}, {"chroma_strength": 1.0}, {"contrast_strength": 1.0}, {"wrap_strength": 1.0}, {"wrap_sigma": 16.0},
               {"wrap_sigma": 0.01}, {"wrap_strength": 0.0, "wrap_sigma": nan}):
        emu.harmonize(fg[:1, :8, :12].contiguous(), a[:1, :8, :12].contiguous(), bg[:1, :8, :12].contiguous(), **dict(good, **kw))
    for args in ((fg[..., :2], a, bg), (fg, a[:, :19], bg), (fg, a, bg[:, :19]), (fg, a, torch.rand(3, 20, 24, 3)), (fg[0], a[0], bg[0])):
        with pytest.raises(ValueError):
            emu.harmonize(*args)
    out, fgo, m = torch.full((2, 20, 24, 3), -7.0), torch.full((2, 20, 24, 3), -7.0), torch.full((2, 12), -7.0)

    def raw(B=2, H=20, W=24, bg_batch=2, **kw):
        p = dict(good, **kw)
        return emu.lib.sdm_harmonize(emu.h, _ptr(fg), _ptr(a), _ptr(bg), bg_batch, B, H, W, p["luma_strength"], p["chroma_strength"], p["contrast_strength"],
                                     p["wrap_strength"], p["wrap_sigma"], _ptr(out), _ptr(fgo), _ptr(m), 0, None)
    emu.lib.kernel_counts(reset=True)
    for kw in bad:
        assert raw(**kw) == -1 and next(iter(kw)).encode() in emu.lib.sdm_last_error(emu.h), kw
    assert raw(bg_batch=3) == -1 and b"bg_batch" in emu.lib.sdm_last_error(emu.h)
    assert raw(bg_batch=0) == -1 and b"bg_batch" in emu.lib.sdm_last_error(emu.h)
    assert raw(H=0) == -1 and raw(W=0) == -1 and raw(B=0) == -1 and b"bad image size" in emu.lib.sdm_last_error(emu.h)
    assert raw(H=32769) == -1 and b"too large" in emu.lib.sdm_last_error(emu.h)
    assert emu.lib.kernel_counts() == {} and all(bool((t == -7.0).all()) for t in (out, fgo, m))      # nothing queued or written
    assert raw() == 0
    want = emu.harmonize(fg, a, bg, **good, return_fg=True, return_map=True)
    assert all(torch.equal(x, y) for x, y in zip((out, fgo, m), want))
    assert raw(bg_batch=1) == 0 and torch.equal(out, emu.harmonize(fg, a, bg[:1].contiguous(), **good))
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    assert raw() == 0                      # host pointers: 3 + 1 + 3 floats per pixel staged in, 3 + 3 staged out, and the plane T of 4 in the arena
    assert emu.resident_bytes() >= emu.weight_bytes() + 2 * 20 * 24 * 4 * (7 + 6 + 4)
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    emu.harmonize(fg, a, bg)                                                # ... and the next call allocates again
