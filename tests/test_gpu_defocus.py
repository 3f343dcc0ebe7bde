"""Background defocus on the MI355X (csrc/k_defocus.h through sdm_defocus_background) against the numpy reference of tests/defocus_suite.py under its
tolerance rule.  No weights, no oracle forward: the file stays cheap (ratios and durations in profiles/NOTES.md)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

LAUNCHES = ("dof_prefix", "dof_gather")      # include/sdmatte.h: two launches per call, whatever the arguments


@pytest.fixture(scope="module")
def bare_engine(pkg):
    """An engine that never loads weights: sdm_defocus_background needs none."""
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)
    yield eng
    eng.close()


def _t(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)) for a in arrays)


def _cuda(*tensors):
    return tuple(None if t is None else t.cuda() for t in tensors)


def test_gpu_defocus_case_list_device_pointers(bare_engine):
    """Device tensors on torch's current stream (sync=False: the result is read through that stream, as the stream contract promises)."""
    import defocus_suite as DS
    bare_engine.lib.kernel_counts(reset=True)
    DS.check(lambda *p: bare_engine.defocus_background(*p, sync=False), lambda t: t.cuda())
    assert bare_engine.lib.kernel_counts() == {k: len(DS.cases()) for k in LAUNCHES}


def test_gpu_defocus_case_list_host_pointers(bare_engine):
    import defocus_suite as DS
    DS.check(bare_engine.defocus_background, lambda t: t)


def test_gpu_defocus_on_a_side_stream(bare_engine):
    """The inputs are produced on a side stream right before the call and the result consumed on it right after: the engine orders itself on both
    ends."""
    import defocus_suite as DS
    image, alpha, fg, bg = DS.inputs("soft", 3, 2, 150, 260, planes=True)
    scaled = [torch.from_numpy(t) * 0.9 for t in (image, alpha, fg, bg)]
    params = (17, 4.0, 0.5)
    refs = DS.references_for(*(t.numpy() for t in scaled), params)
    base = _cuda(*_t(image, alpha, fg, bg))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        ins = [t * 0.9 for t in base]
        out = bare_engine.defocus_background(*ins, *params, sync=False)
        out2 = out * 1.0
    st.synchronize()
    assert all(torch.equal(d.cpu(), h) for d, h in zip(ins, scaled))
    DS.compare("side_stream_2x150x260", out2, refs)


@pytest.mark.parametrize("H,W,R", [(133, 260, 17), (67, 516, 32), (40, 70, 2), (37, 72, 5)])
def test_gpu_defocus_is_deterministic(bare_engine, H, W, R):
    """Two calls are bit-identical; device pointers and host pointers give the same bits; a batch equals per-image calls; tensors 4 bytes off a 16-byte
    boundary (the scalar load path) give the bits of the aligned ones."""
    import defocus_suite as DS
    host = _t(*DS.inputs("dirty", 7, 3, H, W, planes=True))
    dev = _cuda(*host)
    out = bare_engine.defocus_background(*dev, R, 4.0, 0.5)
    assert torch.equal(out, bare_engine.defocus_background(*dev, R, 4.0, 0.5))
    h = bare_engine.defocus_background(*host, R, 4.0, 0.5)
    assert h.device.type == "cpu" and torch.equal(h, out.cpu())
    for b in range(3):
        assert torch.equal(out[b:b + 1], bare_engine.defocus_background(*(t[b:b + 1].contiguous() for t in dev), R, 4.0, 0.5)), b
    offs = []
    for t in dev:
        buf = torch.empty(t.numel() + 1, device="cuda")
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert t.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 and v.is_contiguous()
        offs.append(v)
    assert torch.equal(out, bare_engine.defocus_background(*offs, R, 4.0, 0.5))
    assert torch.equal(bare_engine.defocus_background(dev[0], dev[1], None, None, R), bare_engine.defocus_background(offs[0], offs[1], None, None, R))


def test_gpu_defocus_identities(bare_engine):
    """a == 1 gives F; a channel with w C == 0 everywhere gives a F (no halo); deep inside a subject larger than the disc the floor keeps out = F."""
    import defocus_suite as DS
    host = _t(*DS.inputs("dirty", 3, 2, 70, 260, planes=True))
    image, alpha, fg, bg = _cuda(*host)
    a = torch.from_numpy(DS.sanitise_alpha(host[1].numpy())).cuda()
    defocus = bare_engine.defocus_background
    out = defocus(image, alpha, fg, bg, 17, 4.0, 0.5)
    assert bool((a == 1.0).any()) and torch.equal(out[a == 1.0], fg[a == 1.0]) and not torch.equal(out, fg)
    assert torch.equal(defocus(image, alpha, None, None, 17)[a == 1.0], image[a == 1.0])
    bg0 = bg.clone(); bg0[..., 1] = 0.0
    assert torch.equal(defocus(image, alpha, fg, bg0, 17, 4.0, 0.5)[..., 1], a * fg[..., 1])
    image, alpha, fg, bg = _cuda(*_t(*DS.inputs("hard", 1, 1, 70, 130, planes=True)))
    out = defocus(image, alpha, fg, bg, 5, 4.0, 0.5)
    assert bool(torch.isfinite(out).all()) and torch.equal(out[alpha == 1.0], fg[alpha == 1.0])


def test_gpu_defocus_2x270x480_and_launch_counts(bare_engine):
    """2 x 270 x 480 at R = 32 with fg, bg and gain against reference(fp64) under the same rule; the per-launch profile shows exactly the two documented
    launches, and the same two at R = 1 without the planes."""
    import defocus_suite as DS
    host = DS.inputs("soft", 21, 2, 270, 480, planes=True)
    params = (32, 4.0, 0.5)
    refs = DS.references_for(*host, params, fast64=True)
    dev = _cuda(*_t(*host))

    def profiled(*args):
        bare_engine.profile(True)
        out = bare_engine.defocus_background(*args)
        bare_engine.profile(False)
        res = bare_engine.profile_results()
        assert {k: v["launches"] for k, v in res.items()} == {k: 1 for k in LAUNCHES}, res
        dump = bare_engine.profile_dump()
        assert all(dump.count("\n" + k) == 1 for k in LAUNCHES)
        return out
    DS.compare("soft_2x270x480_R32_g4_fgbg", profiled(*dev, *params), refs)
    assert bare_engine.last_forward_ms() > 0.0
    profiled(dev[0], dev[1], None, None, 1)


def test_gpu_defocus_serves_its_purpose(bare_engine):
    """No halo: the red of the subject does not reach a single background pixel, while the background did blur; the blur is the closed disc."""
    import defocus_suite as DS
    image, alpha = _cuda(*_t(*DS.purpose_scene()))
    DS.check_purpose(bare_engine.defocus_background(image, alpha, None, None, DS.PURPOSE_R, 0.0, 0.5).cpu().numpy(), "MI355X")
    DS.check_disc_shape(bare_engine.defocus_background, lambda t: t.cuda(), "MI355X")


def test_gpu_defocus_memory_is_counted_and_released(bare_engine):
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    img, a = torch.rand(4, 128, 128, 3), torch.rand(4, 128, 128)
    bare_engine.defocus_background(img, a)
    # host pointers: staging in (3 + 1 floats per pixel) and out (3), and the prefix plane (4) in the arena
    assert bare_engine.resident_bytes() >= bare_engine.weight_bytes() + 4 * 128 * 128 * 4 * (4 + 3 + 4)
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    bare_engine.defocus_background(img.cuda(), a.cuda())
    assert bare_engine.resident_bytes() >= bare_engine.weight_bytes() + 4 * 128 * 128 * 16      # device pointers: the arena plane alone
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    with pytest.raises(ValueError):
        bare_engine.defocus_background(img.cuda(), a.cuda(), radius_px=65)
    with pytest.raises(ValueError):
        bare_engine.defocus_background(img.cuda(), a, radius_px=2)                               # one device for all tensors
    with pytest.raises(ValueError):
        bare_engine.defocus_background(img.cuda(), a.cuda(), bg=img, radius_px=2)
