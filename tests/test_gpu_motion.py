"""Motion-compensated temporal smoothing of the alpha on the MI355X (csrc/k_motion.h through sdm_smooth_alpha_motion) against the numpy reference of
tests/motion_suite.py under its rule.  No weights, no oracle forward: the file stays cheap (ratios and durations in profiles/NOTES.md)."""
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
    """An engine that never loads weights: sdm_smooth_alpha_motion needs none."""
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)
    yield eng
    eng.close()


def _t(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in arrays)


def test_gpu_smooth_motion_case_list_device_pointers(bare_engine):
    """Device tensors on torch's current stream (sync=False: the result is read through that stream, as the stream contract promises)."""
    import motion_suite as MS
    bare_engine.lib.kernel_counts(reset=True)
    MS.check(lambda im, a, *p: bare_engine.smooth_alpha_motion(im, a, *p, sync=False), lambda t: t.cuda())
    assert bare_engine.lib.kernel_counts() == {"tsm_smooth": len(MS.cases())}


def test_gpu_smooth_motion_case_list_host_pointers(bare_engine):
    import motion_suite as MS
    MS.check(lambda im, a, *p: bare_engine.smooth_alpha_motion(im, a, *p), lambda t: t)


def test_gpu_smooth_motion_on_a_side_stream(bare_engine):
    """Frames and alpha are produced on a side stream right before the call and the result consumed on it right after: the engine orders itself on
    both ends."""
    import motion_suite as MS
    image, alpha = MS.inputs("moving", 3, 4, 50, 130)
    scaled = (torch.from_numpy(image) * 0.9, torch.from_numpy(alpha) * 0.9)
    refs = MS.references_for(scaled[0].numpy(), scaled[1].numpy(), MS.PURPOSE)
    base_i, base_a = torch.from_numpy(image).cuda(), torch.from_numpy(alpha).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        im, al = base_i * 0.9, base_a * 0.9
        out = bare_engine.smooth_alpha_motion(im, al, sync=False)
        out2 = out * 1.0
    st.synchronize()
    assert torch.equal(im.cpu(), scaled[0]) and torch.equal(al.cpu(), scaled[1])
    MS.compare("side_stream_4x50x130", out2, refs)


@pytest.mark.parametrize("H,W,radius,patch,search,L", [(67, 130, 2, 1, 4, 3), (40, 517, 1, 0, 8, 4), (67, 130, 4, 2, 2, 5), (40, 517, 2, 2, 3, 2)])
def test_gpu_smooth_motion_is_deterministic(bare_engine, H, W, radius, patch, search, L):
    """Two calls are bit-identical; device pointers and host pointers give the same bits; clip_len = L equals one call per clip (7 frames: the last
    clip is shorter); tensors 4 bytes off a 16-byte boundary (the scalar load path) give the bits of the aligned ones."""
    import motion_suite as MS
    image, alpha = _t(*MS.inputs("dirty", 7, 7, H, W))
    di, da = image.cuda(), alpha.cuda()
    smooth = bare_engine.smooth_alpha_motion
    out = smooth(di, da, radius, patch, search)
    assert torch.equal(out, smooth(di, da, radius, patch, search))
    host = smooth(image, alpha, radius, patch, search)
    assert host.device.type == "cpu" and torch.equal(host, out.cpu())
    clips = smooth(di, da, radius, patch, search, clip_len=L)
    assert not torch.equal(clips, out)
    for lo in range(0, 7, L):
        assert torch.equal(clips[lo:lo + L], smooth(di[lo:lo + L].contiguous(), da[lo:lo + L].contiguous(), radius, patch, search)), lo
    buf_i, buf_a = torch.empty(image.numel() + 1, device="cuda"), torch.empty(alpha.numel() + 1, device="cuda")
    off_i, off_a = buf_i[1:].view(image.shape), buf_a[1:].view(alpha.shape)
    off_i.copy_(di); off_a.copy_(da)
    assert di.data_ptr() % 16 == 0 and off_i.data_ptr() % 16 == 4 and off_a.data_ptr() % 16 == 4 and off_i.is_contiguous()
    assert torch.equal(out, smooth(off_i, off_a, radius, patch, search))


def test_gpu_smooth_motion_identities_and_hard_cut(bare_engine):
    """The no-op conditions return the sanitised alpha bit for bit; a hard cut gives the bits of its two shots."""
    import motion_suite as MS
    image, alpha = _t(*MS.inputs("dirty", 5, 6, 33, 72))
    a = torch.from_numpy(MS.sanitise_alpha(alpha.numpy()))
    di, da = image.cuda(), alpha.cuda()
    smooth = bare_engine.smooth_alpha_motion
    assert not torch.equal(smooth(di, da).cpu(), a)
    assert torch.equal(smooth(di, da, strength=0.0).cpu(), a)
    assert torch.equal(smooth(di, da, max_change=0.0).cpu(), a)
    assert torch.equal(smooth(di, da, clip_len=1).cpu(), a)
    assert torch.equal(smooth(di[:1], da[:1], 4, 2, 8).cpu(), a[:1])
    far = (0.125 * torch.arange(6).float().view(6, 1, 1, 1) + 0.02 * torch.rand(6, 33, 72, 3)).contiguous()
    assert torch.equal(smooth(far.cuda(), da, 4, 2, 4, 0.1).cpu(), a)
    image, alpha = _t(*MS.cut_scene(11, 5, 4, 33, 70))
    di, da = image.cuda(), alpha.cuda()
    out = smooth(di, da, 4, 2, 4)
    assert torch.equal(out[:5], smooth(di[:5], da[:5], 4, 2, 4)) and torch.equal(out[5:], smooth(di[5:].contiguous(), da[5:].contiguous(), 4, 2, 4))
    assert not torch.equal(out.cpu(), torch.from_numpy(MS.sanitise_alpha(alpha.numpy())))


def test_gpu_smooth_motion_search_0_is_the_existing_call(bare_engine):
    """search = 0: the launch and the bits of smooth_alpha_temporal, whatever motion_penalty says."""
    import motion_suite as MS
    image, alpha = _t(*MS.inputs("dirty", 3, 6, 67, 130))
    di, da = image.cuda(), alpha.cuda()
    for radius, patch in ((2, 1), (4, 2)):
        bare_engine.lib.kernel_counts(reset=True)
        out = bare_engine.smooth_alpha_motion(di, da, radius, patch, 0, motion_penalty=0.3)
        assert bare_engine.lib.kernel_counts() == {"ts_smooth": 1}
        assert torch.equal(out, bare_engine.smooth_alpha_temporal(di, da, radius, patch))


def test_gpu_smooth_motion_4x135x240_and_launch_counts(bare_engine):
    """4 frames of 135 x 240 at radius 2, patch 2, search 4 against reference(fp64) under the same rule; the per-launch profile shows exactly one
    tsm_smooth, and the same one for two clips and for patch 0, search 8."""
    import motion_suite as MS
    image, alpha = MS.inputs("moving", 21, 4, 135, 240)
    params = (2, 2, 4, 0.1, 0.02, 1.0, 1.0, 0)
    refs = MS.references_for(image, alpha, params)
    assert MS.undecided_share(refs) <= MS.MAX_UNDECIDED_SHARE
    image, alpha = torch.from_numpy(image).cuda(), torch.from_numpy(alpha).cuda()

    def profiled(*p):
        bare_engine.profile(True)
        out = bare_engine.smooth_alpha_motion(image, alpha, *p)
        bare_engine.profile(False)
        res = bare_engine.profile_results()
        assert {k: v["launches"] for k, v in res.items()} == {"tsm_smooth": 1}, res
        assert bare_engine.profile_dump().count("\ntsm_smooth") == 1
        return out
    MS.compare("moving_4x135x240_r2_p2_s4", profiled(*params), refs)
    assert bare_engine.last_forward_ms() > 0.0
    profiled(2, 2, 4, 0.1, 0.02, 1.0, 1.0, 2)
    profiled(1, 0, 8)


def test_gpu_smooth_motion_translation(bare_engine):
    import motion_suite as MS
    MS.check_translation(lambda im, a, *p: bare_engine.smooth_alpha_motion(im, a, *p), lambda t: t.cuda(), "MI355X")


def test_gpu_smooth_motion_serves_its_purpose(bare_engine):
    """The soft edge of a subject moving 2 pixels per frame stops shimmering (band flicker at most 0.55 x the observed alpha's, where the existing filter
    leaves 0.87 x) without being smeared (band mean error at most 0.85 x, largest error at most the observed one)."""
    import motion_suite as MS
    image, _, obs = MS.purpose_scene()
    out = bare_engine.smooth_alpha_motion(torch.from_numpy(image).cuda(), torch.from_numpy(obs).cuda(), *MS.PURPOSE)
    MS.check_purpose(out.cpu().numpy(), "MI355X")


def test_gpu_smooth_motion_memory_is_counted_and_released(bare_engine):
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    img, a = torch.rand(4, 64, 128, 3), torch.rand(4, 64, 128)
    bare_engine.smooth_alpha_motion(img, a, search=2)
    assert bare_engine.resident_bytes() >= bare_engine.weight_bytes() + 4 * 64 * 128 * 4 * 5      # host pointers: staging in (3 + 1) and out (1)
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    with pytest.raises(ValueError):
        bare_engine.smooth_alpha_motion(img.cuda(), a.cuda(), search=9)
    with pytest.raises(ValueError):
        bare_engine.smooth_alpha_motion(img.cuda(), a, 2)                                        # one device for all tensors
