"""Foreground estimation on the MI355X (csrc/k_foreground.h through sdm_estimate_foreground) against the numpy reference of
tests/foreground_suite.py under its tolerance rule.  No weights, no oracle forward: the file stays cheap (durations in profiles/NOTES.md)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def bare_engine(pkg):
    """An engine that never loads weights: sdm_estimate_foreground needs none."""
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)
    yield eng
    eng.close()


def test_gpu_estimate_foreground_case_list_device_pointers(bare_engine):
    """Device tensors on torch's current stream (sync=False: the result is read through that stream, as the stream contract promises)."""
    import foreground_suite as FS
    FS.check(lambda im, a, p, rgba: bare_engine.estimate_foreground(im, a, rgba=rgba, sync=False, **p), lambda t: t.cuda())


def test_gpu_estimate_foreground_case_list_host_pointers(bare_engine):
    import foreground_suite as FS
    FS.check(lambda im, a, p, rgba: bare_engine.estimate_foreground(im, a, rgba=rgba, **p), lambda t: t)


def test_gpu_estimate_foreground_on_a_side_stream(bare_engine):
    """Image and alpha are produced on a side stream right before the call and the colours consumed on it right after: the engine orders itself on
    both ends."""
    import foreground_suite as FS
    image, alpha, _, _ = FS.scene(3, 1, 300, 500)
    scaled = (torch.from_numpy(image) * 0.9, torch.from_numpy(alpha) * 0.9)
    refs = FS.references_for(scaled[0].numpy(), scaled[1].numpy(), {})
    base_i, base_a = torch.from_numpy(image).cuda(), torch.from_numpy(alpha).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        im, al = base_i * 0.9, base_a * 0.9
        fg, bg = bare_engine.estimate_foreground(im, al, sync=False)
        fg2, bg2 = fg * 1.0, bg * 1.0
    st.synchronize()
    assert torch.equal(im.cpu(), scaled[0]) and torch.equal(al.cpu(), scaled[1])
    FS.compare("side_stream_300x500", fg2, bg2, scaled[1].numpy(), refs, False)


def test_gpu_estimate_foreground_is_deterministic(bare_engine):
    """Two calls are bit-identical; B = 3 equals three single calls; device pointers and host pointers give the same bits; want_background=False
    and rgba leave the foreground's bits alone."""
    import foreground_suite as FS
    image, alpha, _, _ = FS.scene(7, 3, 333, 517)
    rng = np.random.default_rng(7)
    alpha[2] = rng.uniform(size=alpha[2].shape)                          # one image whose every pixel moves in every step
    image, alpha = torch.from_numpy(image), torch.from_numpy(alpha)
    fg, bg = bare_engine.estimate_foreground(image.cuda(), alpha.cuda())
    fg_b, bg_b = bare_engine.estimate_foreground(image.cuda(), alpha.cuda())
    assert torch.equal(fg, fg_b) and torch.equal(bg, bg_b)
    for b in range(3):
        f1, b1 = bare_engine.estimate_foreground(image[b:b + 1].cuda(), alpha[b:b + 1].cuda())
        assert torch.equal(fg[b:b + 1], f1) and torch.equal(bg[b:b + 1], b1), b
    fh, bh = bare_engine.estimate_foreground(image, alpha)
    assert fh.device.type == "cpu" and torch.equal(fh, fg.cpu()) and torch.equal(bh, bg.cpu())
    f4, none = bare_engine.estimate_foreground(image.cuda(), alpha.cuda(), rgba=True, want_background=False)
    assert none is None and torch.equal(f4[..., :3], fg) and torch.equal(f4[..., 3].cpu(), alpha)


def test_gpu_estimate_foreground_1080p_and_launch_counts(bare_engine):
    """One 1080 x 1920 image against reference(fp64) under the same rule; the per-launch profile shows 1 + 6 launches."""
    import foreground_suite as FS
    image, alpha, _, _ = FS.scene(21, 1, 1080, 1920)
    refs = FS.references_for(image, alpha, {})
    bare_engine.profile(True)
    fg, bg = bare_engine.estimate_foreground(torch.from_numpy(image).cuda(), torch.from_numpy(alpha).cuda(), rgba=True)
    bare_engine.profile(False)
    FS.compare("soft_1080x1920", fg, bg, alpha, refs, True)
    res = bare_engine.profile_results()
    assert res["fg_small"]["launches"] == 1 and res["fg_level"]["launches"] == 6 == FS.n_large_levels(1080, 1920), sorted(res)
    assert "fg_small," in bare_engine.profile_dump() and "fg_level," in bare_engine.profile_dump()
    assert bare_engine.last_forward_ms() > 0.0


def test_gpu_estimate_foreground_memory_is_counted_and_released(bare_engine):
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    img, a = torch.rand(1, 256, 256, 3), torch.rand(1, 256, 256)
    bare_engine.estimate_foreground(img.cuda(), a.cuda())
    mid = bare_engine.resident_bytes()
    assert mid >= bare_engine.weight_bytes() + (128 * 128 + 64 * 64 + 32 * 32) * 32      # the level planes live in the arena
    bare_engine.estimate_foreground(img, a)
    assert bare_engine.resident_bytes() >= mid + 256 * 256 * 4 * (3 + 1 + 3 + 3)        # host pointers: staging in and out
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    with pytest.raises(ValueError):
        bare_engine.estimate_foreground(img.cuda(), a.cuda(), n_big_iters=5)
    with pytest.raises(ValueError):
        bare_engine.estimate_foreground(img.cuda(), a)                   # one device for all tensors
