"""Guided alpha refinement on the MI355X (csrc/k_guided.h through sdm_refine_alpha_guided) against the numpy reference of tests/guided_suite.py under
its tolerance rule.  No weights, no oracle forward: the file stays cheap (ratios and durations in profiles/NOTES.md)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

LAUNCHES = {"gf_mean": 1, "gf_fit": 1, "gf_smooth": 1, "gf_apply": 1}      # the launch count stated in csrc/k_guided.h and include/sdmatte.h


@pytest.fixture(scope="module")
def bare_engine(pkg):
    """An engine that never loads weights: sdm_refine_alpha_guided needs none."""
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)
    yield eng
    eng.close()


def test_gpu_refine_alpha_case_list_device_pointers(bare_engine):
    """Device tensors on torch's current stream (sync=False: the result is read through that stream, as the stream contract promises)."""
    import guided_suite as GS
    GS.check(lambda im, a, s, r, eps: bare_engine.refine_alpha_guided(im, a, s, r, eps, sync=False), lambda t: t.cuda())


def test_gpu_refine_alpha_case_list_host_pointers(bare_engine):
    import guided_suite as GS
    GS.check(lambda im, a, s, r, eps: bare_engine.refine_alpha_guided(im, a, s, r, eps), lambda t: t)


def test_gpu_refine_alpha_on_a_side_stream(bare_engine):
    """Image and alpha are produced on a side stream right before the call and the result consumed on it right after: the engine orders itself on
    both ends."""
    import guided_suite as GS
    image, alpha = GS._inputs("soft", 3, 1, 300, 500)
    scaled = (torch.from_numpy(image) * 0.9, torch.from_numpy(alpha) * 0.9)
    refs = GS.references_for(scaled[0].numpy(), scaled[1].numpy(), (4, 2, 1e-4))
    base_i, base_a = torch.from_numpy(image).cuda(), torch.from_numpy(alpha).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        im, al = base_i * 0.9, base_a * 0.9
        out = bare_engine.refine_alpha_guided(im, al, 4, sync=False)
        out2 = out * 1.0
    st.synchronize()
    assert torch.equal(im.cpu(), scaled[0]) and torch.equal(al.cpu(), scaled[1])
    GS.compare("side_stream_300x500", out2, refs)


@pytest.mark.parametrize("H,W,s,radius", [(333, 517, 4, 2), (334, 516, 2, 3), (120, 256, 1, 5), (333, 517, 3, 32)])
def test_gpu_refine_alpha_is_deterministic(bare_engine, H, W, s, radius):
    """Two calls are bit-identical; B = 3 equals three single calls (H W no multiple of 4: the images start inside a run of 4 pixels); device pointers
    and host pointers give the same bits."""
    import guided_suite as GS
    image, alpha = GS._inputs("soft", 7, 3, H, W)
    alpha[2] = np.random.default_rng(7).uniform(size=alpha[2].shape)
    image, alpha = torch.from_numpy(image), torch.from_numpy(alpha)
    out = bare_engine.refine_alpha_guided(image.cuda(), alpha.cuda(), s, radius)
    assert torch.equal(out, bare_engine.refine_alpha_guided(image.cuda(), alpha.cuda(), s, radius))
    for b in range(3):
        assert torch.equal(out[b:b + 1], bare_engine.refine_alpha_guided(image[b:b + 1].cuda(), alpha[b:b + 1].cuda(), s, radius)), b
    host = bare_engine.refine_alpha_guided(image, alpha, s, radius)
    assert host.device.type == "cpu" and torch.equal(host, out.cpu())


def test_gpu_refine_alpha_540x960_and_launch_counts(bare_engine):
    """One 540 x 960 image with s = 4 against reference(fp64) under the same rule; the per-launch profile shows the documented four launches, and
    the same four for B = 2 and for radius 32."""
    import guided_suite as GS
    image, alpha = GS._inputs("soft", 21, 1, 540, 960)
    refs = GS.references_for(image, alpha, (4, 2, 1e-4))
    image, alpha = torch.from_numpy(image).cuda(), torch.from_numpy(alpha).cuda()

    def profiled(im, al, radius):
        bare_engine.profile(True)
        out = bare_engine.refine_alpha_guided(im, al, 4, radius)
        bare_engine.profile(False)
        res = bare_engine.profile_results()
        assert {k: v["launches"] for k, v in res.items()} == LAUNCHES, res
        assert bare_engine.profile_dump().count("\ngf_") == sum(LAUNCHES.values())
        return out
    GS.compare("soft_540x960_s4_r2", profiled(image, alpha, 2), refs)
    assert bare_engine.last_forward_ms() > 0.0
    profiled(torch.cat([image, image]), torch.cat([alpha, alpha]), 2)
    profiled(image, alpha, 32)


def test_gpu_refine_alpha_serves_its_purpose(bare_engine):
    """The 2-pixel edge that a reduction by 4 blurred comes back: at most half the bilinear alpha's max error, and no larger mean error."""
    import guided_suite as GS
    image, _, blurred = GS.purpose_scene()
    out = bare_engine.refine_alpha_guided(torch.from_numpy(image).cuda(), torch.from_numpy(blurred).cuda(), *GS.PURPOSE)
    GS.check_purpose(out.cpu().numpy(), "MI355X")


def test_gpu_refine_alpha_memory_is_counted_and_released(bare_engine):
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    img, a = torch.rand(1, 256, 256, 3), torch.rand(1, 256, 256)
    bare_engine.refine_alpha_guided(img.cuda(), a.cuda(), 2)
    mid = bare_engine.resident_bytes()
    assert mid >= bare_engine.weight_bytes() + 128 * 128 * 4 * 8                         # the a, b, abar, bbar planes live in the arena
    bare_engine.refine_alpha_guided(img, a, 2)
    assert bare_engine.resident_bytes() >= mid + 256 * 256 * 4 * 5                       # host pointers: staging in (3 + 1) and out (1)
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    with pytest.raises(ValueError):
        bare_engine.refine_alpha_guided(img.cuda(), a.cuda(), 17)
    with pytest.raises(ValueError):
        bare_engine.refine_alpha_guided(img.cuda(), a, 2)                                # one device for all tensors
