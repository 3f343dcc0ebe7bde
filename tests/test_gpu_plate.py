"""The clean plate on the MI355X (csrc/k_plate.h through sdm_fill_background) against the numpy reference of tests/plate_suite.py under its tolerance
rule.  No weights, no oracle forward: the file stays cheap (ratios and durations in profiles/NOTES.md)."""
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
    """An engine that never loads weights: sdm_fill_background needs none."""
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)
    yield eng
    eng.close()


def _t(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)) for a in arrays)


def _cuda(*tensors):
    return tuple(None if t is None else t.cuda() for t in tensors)


def test_gpu_plate_case_list_device_pointers(bare_engine):
    """Device tensors on torch's current stream (sync=False: the result is read through that stream, as the stream contract promises); the launch
    counts of the whole run follow the header's formula."""
    import plate_suite as PS
    bare_engine.lib.kernel_counts(reset=True)
    PS.check(lambda *p: bare_engine.fill_background(*p, sync=False), lambda t: t.cuda())
    assert bare_engine.lib.kernel_counts() == PS.case_launches()


def test_gpu_plate_case_list_host_pointers(bare_engine):
    import plate_suite as PS
    PS.check(bare_engine.fill_background, lambda t: t)


def test_gpu_plate_on_a_side_stream(bare_engine):
    """The inputs are produced on a side stream right before the call and the result consumed on it right after: the engine orders itself on both
    ends."""
    import plate_suite as PS
    arrays = PS.inputs("soft", 3, 2, 150, 260, with_bg=True, with_hole=True)
    scaled = [torch.from_numpy(t) * 0.9 for t in arrays]
    refs = PS.references_for(*(t.numpy() for t in scaled), 0.25)
    base = _cuda(*_t(*arrays))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        ins = [t * 0.9 for t in base]
        out = bare_engine.fill_background(*ins, 0.25, sync=False)
        out2 = out * 1.0
    st.synchronize()
    same = lambda d, h: torch.equal(torch.nan_to_num(d, nan=-9.0), torch.nan_to_num(h, nan=-9.0))      # (the hole plane carries a NaN)
    assert all(same(d.cpu(), h) for d, h in zip(ins, scaled))
    PS.compare("side_stream_2x150x260", out2, refs)


@pytest.mark.parametrize("H,W", [(133, 260), (67, 131), (40, 72), (20, 24)])
def test_gpu_plate_is_deterministic(bare_engine, H, W):
    """Two calls are bit-identical; device pointers and host pointers give the same bits; a batch equals per-image calls; tensors 4 bytes off a 16-byte
    boundary (the scalar load path) give the bits of the aligned ones."""
    import plate_suite as PS
    host = _t(*PS.inputs("dirty", 7, 3, H, W, with_bg=True, with_hole=True))
    dev = _cuda(*host)
    fill = bare_engine.fill_background
    out = fill(*dev, 0.25)
    assert torch.equal(out, fill(*dev, 0.25))
    h = fill(*host, 0.25)
    assert h.device.type == "cpu" and torch.equal(h, out.cpu())
    for b in range(3):
        assert torch.equal(out[b:b + 1], fill(*(t[b:b + 1].contiguous() for t in dev), 0.25)), b
    offs = []
    for t in dev:
        buf = torch.empty(t.numel() + 1, device="cuda")
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert t.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 and v.is_contiguous()
        offs.append(v)
    assert torch.equal(out, fill(*offs, 0.25))
    assert torch.equal(out, fill(dev[0], dev[1], dev[2], offs[3], 0.25))
    assert torch.equal(fill(dev[0], dev[1]), fill(offs[0], offs[1]))


@pytest.mark.parametrize("H,W", [(67, 131), (40, 72), (20, 24)])
def test_gpu_plate_identities(bare_engine, H, W):
    """w_0 == 1 gives C; a channel that is 0 wherever w_0 > 0 stays 0; a flat background behind a hard alpha gives exactly 0.5: bit for bit, on device
    tensors."""
    import plate_suite as PS
    PS.check_identities(bare_engine.fill_background, lambda t: t.cuda(), H, W, "MI355X")


def test_gpu_plate_all_subject_gives_zeros(bare_engine):
    import plate_suite as PS
    image, alpha, _, _ = _cuda(*_t(*PS.inputs("soft", 5, 2, 70, 90)))
    alpha[0] = 1.0
    out = bare_engine.fill_background(image, alpha)
    assert bool((out[0] == 0.0).all()) and bool((out[1] != 0.0).any())


def test_gpu_plate_2x270x480_and_launch_counts(bare_engine):
    """2 x 270 x 480 with bg and hole against reference(fp64) under the same rule; the per-launch profile shows exactly the documented launches (S = 4:
    two pulls, the small kernel, two pushes), and the one launch of a 32 x 32 call."""
    import plate_suite as PS
    host = PS.inputs("soft", 21, 2, 270, 480, with_bg=True, with_hole=True)
    refs = PS.references_for(*host, 0.25)
    dev = _cuda(*_t(*host))

    def profiled(want, *args):
        bare_engine.profile(True)
        out = bare_engine.fill_background(*args)
        bare_engine.profile(False)
        res = bare_engine.profile_results()
        assert {k: v["launches"] for k, v in res.items()} == want, res
        dump = bare_engine.profile_dump()
        assert all(dump.count("\n" + k) == n for k, n in want.items())
        return out
    assert PS.launches(270, 480) == {"plate_pull": 2, "plate_small": 1, "plate_push": 2}
    PS.compare("soft_2x270x480_cut0.25_bg_hole", profiled(PS.launches(270, 480), *dev, 0.25), refs)
    assert bare_engine.last_forward_ms() > 0.0
    profiled({"plate_small": 1}, dev[0][:, :32, :32].contiguous(), dev[1][:, :32, :32].contiguous())


def test_gpu_plate_serves_its_purpose(bare_engine):
    """The subject's red reaches no pixel of the plate, and the fill is as close to the true background as the reference's."""
    import plate_suite as PS
    PS.check_purpose(bare_engine.fill_background, lambda t: t.cuda(), "MI355X")


def test_gpu_plate_memory_is_counted_and_released(bare_engine):
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    img, a = torch.rand(4, 128, 128, 3), torch.rand(4, 128, 128)
    bare_engine.fill_background(img, a)
    # host pointers: staging in (3 + 1 floats per pixel) and out (3), and level 1 of the pyramid (4 floats per 4 pixels) in the arena
    assert bare_engine.resident_bytes() >= bare_engine.weight_bytes() + 4 * 128 * 128 * 4 * (4 + 3 + 1)
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    bare_engine.fill_background(img.cuda(), a.cuda())
    assert bare_engine.resident_bytes() >= bare_engine.weight_bytes() + 4 * 64 * 64 * 16       # device pointers: the pyramid alone
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    with pytest.raises(ValueError):
        bare_engine.fill_background(img.cuda(), a.cuda(), alpha_cut=1.5)
    with pytest.raises(ValueError):
        bare_engine.fill_background(img.cuda(), a, alpha_cut=0.5)                                # one device for all tensors
    with pytest.raises(ValueError):
        bare_engine.fill_background(img.cuda(), a.cuda(), bg=img)
    with pytest.raises(ValueError):
        bare_engine.fill_background(img.cuda(), a.cuda(), hole=a)
