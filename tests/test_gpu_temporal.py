"""Temporal smoothing of the alpha on the MI355X (csrc/k_temporal.h through sdm_smooth_alpha_temporal) against the numpy reference of
tests/temporal_suite.py under its tolerance rule.  No weights, no oracle forward: the file stays cheap (ratios and durations in profiles/NOTES.md)."""
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
    """An engine that never loads weights: sdm_smooth_alpha_temporal needs none."""
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)
    yield eng
    eng.close()


def _t(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in arrays)


def test_gpu_smooth_alpha_case_list_device_pointers(bare_engine):
    """Device tensors on torch's current stream (sync=False: the result is read through that stream, as the stream contract promises)."""
    import temporal_suite as TS
    bare_engine.lib.kernel_counts(reset=True)
    TS.check(lambda im, a, *p: bare_engine.smooth_alpha_temporal(im, a, *p, sync=False), lambda t: t.cuda())
    assert bare_engine.lib.kernel_counts() == {"ts_smooth": len(TS.cases())}


def test_gpu_smooth_alpha_case_list_host_pointers(bare_engine):
    import temporal_suite as TS
    TS.check(lambda im, a, *p: bare_engine.smooth_alpha_temporal(im, a, *p), lambda t: t)


def test_gpu_smooth_alpha_on_a_side_stream(bare_engine):
    """Frames and alpha are produced on a side stream right before the call and the result consumed on it right after: the engine orders itself on
    both ends."""
    import temporal_suite as TS
    image, alpha = TS._inputs("moving", 3, 6, 150, 260)
    scaled = (torch.from_numpy(image) * 0.9, torch.from_numpy(alpha) * 0.9)
    refs = TS.references_for(scaled[0].numpy(), scaled[1].numpy(), TS.PURPOSE)
    base_i, base_a = torch.from_numpy(image).cuda(), torch.from_numpy(alpha).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        im, al = base_i * 0.9, base_a * 0.9
        out = bare_engine.smooth_alpha_temporal(im, al, sync=False)
        out2 = out * 1.0
    st.synchronize()
    assert torch.equal(im.cpu(), scaled[0]) and torch.equal(al.cpu(), scaled[1])
    TS.compare("side_stream_6x150x260", out2, refs)


@pytest.mark.parametrize("H,W,radius,patch,L", [(133, 260, 2, 1, 3), (67, 130, 4, 2, 5), (40, 517, 1, 0, 4), (37, 72, 3, 2, 2)])
def test_gpu_smooth_alpha_is_deterministic(bare_engine, H, W, radius, patch, L):
    """Two calls are bit-identical; device pointers and host pointers give the same bits; clip_len = L equals one call per clip (11 frames: the last
    clip is shorter); tensors 4 bytes off a 16-byte boundary (the scalar load path) give the bits of the aligned ones."""
    import temporal_suite as TS
    image, alpha = _t(*TS._inputs("dirty", 7, 11, H, W))
    di, da = image.cuda(), alpha.cuda()
    out = bare_engine.smooth_alpha_temporal(di, da, radius, patch)
    assert torch.equal(out, bare_engine.smooth_alpha_temporal(di, da, radius, patch))
    host = bare_engine.smooth_alpha_temporal(image, alpha, radius, patch)
    assert host.device.type == "cpu" and torch.equal(host, out.cpu())
    clips = bare_engine.smooth_alpha_temporal(di, da, radius, patch, clip_len=L)
    assert not torch.equal(clips, out)
    for lo in range(0, 11, L):
        assert torch.equal(clips[lo:lo + L], bare_engine.smooth_alpha_temporal(di[lo:lo + L].contiguous(), da[lo:lo + L].contiguous(), radius, patch)), lo
    buf_i, buf_a = torch.empty(image.numel() + 1, device="cuda"), torch.empty(alpha.numel() + 1, device="cuda")
    off_i, off_a = buf_i[1:].view(image.shape), buf_a[1:].view(alpha.shape)
    off_i.copy_(di); off_a.copy_(da)
    assert di.data_ptr() % 16 == 0 and off_i.data_ptr() % 16 == 4 and off_a.data_ptr() % 16 == 4 and off_i.is_contiguous()
    assert torch.equal(out, bare_engine.smooth_alpha_temporal(off_i, off_a, radius, patch))


def test_gpu_smooth_alpha_identities_and_hard_cut(bare_engine):
    """The no-op conditions return the sanitised alpha bit for bit; a hard cut gives the bits of its two shots."""
    import temporal_suite as TS
    image, alpha = _t(*TS._inputs("dirty", 5, 6, 33, 72))
    a = torch.from_numpy(TS.sanitise_alpha(alpha.numpy()))
    di, da = image.cuda(), alpha.cuda()
    smooth = bare_engine.smooth_alpha_temporal
    assert not torch.equal(smooth(di, da).cpu(), a)
    assert torch.equal(smooth(di, da, strength=0.0).cpu(), a)
    assert torch.equal(smooth(di, da, max_change=0.0).cpu(), a)
    assert torch.equal(smooth(di, da, clip_len=1).cpu(), a)
    assert torch.equal(smooth(di[:1], da[:1], 4, 2).cpu(), a[:1])
    far = (0.125 * torch.arange(6).float().view(6, 1, 1, 1) + 0.02 * torch.rand(1, 33, 72, 3)).expand(6, 33, 72, 3).contiguous()
    assert torch.equal(smooth(far.cuda(), da, 4, 2, 0.1).cpu(), a)
    image, alpha = _t(*TS.cut_scene(11, 5, 4, 33, 70))
    di, da = image.cuda(), alpha.cuda()
    out = smooth(di, da, 4, 2)
    assert torch.equal(out[:5], smooth(di[:5], da[:5], 4, 2)) and torch.equal(out[5:], smooth(di[5:].contiguous(), da[5:].contiguous(), 4, 2))


def test_gpu_smooth_alpha_6x270x480_and_launch_counts(bare_engine):
    """6 frames of 270 x 480 at radius 4, patch 2 against reference(fp64) under the same rule; the per-launch profile shows the one documented launch,
    and the same one for two clips and for radius 1, patch 0."""
    import temporal_suite as TS
    image, alpha = TS._inputs("moving", 21, 6, 270, 480)
    params = (4, 2, 0.1, 1.0, 1.0, 0)
    refs = TS.references_for(image, alpha, params)
    image, alpha = torch.from_numpy(image).cuda(), torch.from_numpy(alpha).cuda()

    def profiled(*p):
        bare_engine.profile(True)
        out = bare_engine.smooth_alpha_temporal(image, alpha, *p)
        bare_engine.profile(False)
        res = bare_engine.profile_results()
        assert {k: v["launches"] for k, v in res.items()} == {"ts_smooth": 1}, res
        assert bare_engine.profile_dump().count("\nts_smooth") == 1
        return out
    TS.compare("moving_6x270x480_r4_p2", profiled(*params), refs)
    assert bare_engine.last_forward_ms() > 0.0
    profiled(4, 2, 0.1, 1.0, 1.0, 3)
    profiled(1, 0)


def test_gpu_smooth_alpha_serves_its_purpose(bare_engine):
    """The shimmer of a per-frame alpha over a static background goes (flicker at most half), and a subject moving 3 pixels per frame is not smeared
    (mean and max error stay those of the observed alpha)."""
    import temporal_suite as TS
    image, _, obs = TS.purpose_scene()
    out = bare_engine.smooth_alpha_temporal(torch.from_numpy(image).cuda(), torch.from_numpy(obs).cuda(), *TS.PURPOSE)
    TS.check_purpose(out.cpu().numpy(), "MI355X")


def test_gpu_smooth_alpha_memory_is_counted_and_released(bare_engine):
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    img, a = torch.rand(4, 128, 128, 3), torch.rand(4, 128, 128)
    bare_engine.smooth_alpha_temporal(img, a)
    assert bare_engine.resident_bytes() >= bare_engine.weight_bytes() + 4 * 128 * 128 * 4 * 5      # host pointers: staging in (3 + 1) and out (1)
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    with pytest.raises(ValueError):
        bare_engine.smooth_alpha_temporal(img.cuda(), a.cuda(), 5)
    with pytest.raises(ValueError):
        bare_engine.smooth_alpha_temporal(img.cuda(), a, 2)                                      # one device for all tensors
