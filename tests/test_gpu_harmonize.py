"""Harmonize on the MI355X (csrc/k_harmonize.h through sdm_harmonize) against the numpy reference of tests/harmonize_suite.py under its tolerance rule.
No weights, no oracle forward: the file stays cheap (ratios and durations in profiles/NOTES.md)."""
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
    """An engine that never loads weights: sdm_harmonize needs none."""
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)
    yield eng
    eng.close()


def _t(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in arrays)


def _cuda(*tensors):
    return tuple(t.cuda() for t in tensors)


def _full(eng, **kw):
    return lambda *p: eng.harmonize(*p, return_fg=True, return_map=True, **kw)


def _same(xs, ys):
    return all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(xs, ys))


def test_gpu_harmonize_case_list_device_pointers(bare_engine):
    """Device tensors on torch's current stream (sync=False: the results are read through that stream, as the stream contract promises); the launch
    counts of the whole run are the stages that are on, case by case."""
    import harmonize_suite as HS
    bare_engine.lib.kernel_counts(reset=True)
    HS.check(_full(bare_engine, sync=False), lambda t: t.cuda())
    assert bare_engine.lib.kernel_counts() == HS.expected_counts([c[4] for c in HS.cases()])


def test_gpu_harmonize_case_list_host_pointers(bare_engine):
    import harmonize_suite as HS
    HS.check(_full(bare_engine), lambda t: t)


def test_gpu_harmonize_on_a_side_stream(bare_engine):
    """The inputs are produced on a side stream right before the call and the results consumed on it right after: the engine orders itself on both ends."""
    import harmonize_suite as HS
    fg, alpha, bg = HS.inputs("soft", 3, 2, 150, 260)
    scaled = [torch.from_numpy(t) * 0.9 for t in (fg, alpha, bg)]
    params = (0.6, 0.8, 0.5, 0.5, 6.0)
    refs = HS.references_for(*(t.numpy() for t in scaled), params, fast64=True)
    base = _cuda(*_t(fg, alpha, bg))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        ins = [t * 0.9 for t in base]
        got = _full(bare_engine, sync=False)(*ins, *params)
        got2 = [t * 1.0 for t in got]
    st.synchronize()
    assert all(torch.equal(d.cpu(), h) for d, h in zip(ins, scaled))
    HS.compare("side_stream_2x150x260", got2, refs)


@pytest.mark.parametrize("H,W,sigma", [(133, 260, 6.0), (67, 516, 16.0), (40, 70, 0.3), (37, 72, 2.0)])
def test_gpu_harmonize_is_deterministic(bare_engine, H, W, sigma):
    """Identities 5 and 6: two calls are bit-identical; device pointers and host pointers give the same bits; a batch equals per-image calls; tensors 4
    bytes off a 16-byte boundary (the scalar load path) give the bits of the aligned ones; one background for the batch equals its copies."""
    import harmonize_suite as HS
    host = _t(*HS.inputs("dirty", 7, 3, H, W))
    dev = _cuda(*host)
    params = (0.6, 0.8, 0.5, 0.5, sigma)
    call = _full(bare_engine)
    got = call(*dev, *params)
    assert _same(got, call(*dev, *params))
    h = call(*host, *params)
    assert all(t.device.type == "cpu" for t in h) and _same(h, got)
    for b in range(3):
        assert _same([t[b:b + 1] for t in got], call(*(t[b:b + 1].contiguous() for t in dev), *params)), b
    offs = []
    for t in dev:
        buf = torch.empty(t.numel() + 1, device="cuda")
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert t.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 and v.is_contiguous()
        offs.append(v)
    assert _same(got, call(*offs, *params))
    assert _same(got, call(dev[0], offs[1], dev[2], *params))
    one_bg = dev[2][:1].contiguous()
    assert _same(call(dev[0], dev[1], one_bg, *params), call(dev[0], dev[1], one_bg.repeat(3, 1, 1, 1), *params))


def test_gpu_harmonize_identities(bare_engine):
    """Identities 1 to 4 of the header, bit for bit."""
    import harmonize_suite as HS
    host = _t(*HS.inputs("dirty", 3, 2, 70, 260))
    fg, alpha, bg = _cuda(*host)
    a = torch.from_numpy(HS.sanitise_alpha(host[1].numpy())).cuda()
    assert bool((a == 1.0).any()) and bool((a == 0.0).any())
    call = _full(bare_engine)
    out, fgo, _ = call(fg, alpha, bg, 0.6, 0.8, 0.5, 0.5, 6.0)
    assert torch.equal(out[a == 0.0], bg[a == 0.0])
    assert torch.equal(out[a == 1.0], fgo[a == 1.0]) and not torch.equal(out, fgo)
    out0, fgo0, m0 = call(fg, alpha, bg, 0.0, 0.0, 0.0, 0.0, 6.0)
    assert torch.equal(fgo0, fg) and torch.equal(out0, a.unsqueeze(-1) * fg + (1.0 - a).unsqueeze(-1) * bg)
    assert torch.equal(m0.cpu(), torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]).repeat(2, 1))
    # 4: deep inside a hard subject the wrap changes nothing, elsewhere it does
    fg, alpha, bg = _t(*HS.inputs("hard", 1, 1, 70, 130))
    sigma = 2.0
    r = HS.wrap_weights(sigma)[0]
    pad = torch.nn.functional.pad(alpha, (r, r, r, r), value=1.0)                    # pixels beyond the frame do not exist
    deep = (-torch.nn.functional.max_pool2d(-pad.unsqueeze(1), 2 * r + 1, 1)[0, 0] == 1.0).numpy()
    assert deep.sum() > 100 and (~deep).sum() > 100
    fg, alpha, bg = _cuda(fg, alpha, bg)
    with_wrap = bare_engine.harmonize(fg, alpha, bg, 0.6, 0.8, 0.5, 0.7, sigma, return_fg=True)[1][0].cpu().numpy()
    without = bare_engine.harmonize(fg, alpha, bg, 0.6, 0.8, 0.5, 0.0, sigma, return_fg=True)[1][0].cpu().numpy()
    assert np.array_equal(with_wrap[deep], without[deep]) and not np.array_equal(with_wrap[~deep], without[~deep])


def test_gpu_harmonize_2x270x480_and_launch_counts(bare_engine):
    """2 x 270 x 480 at sigma = 16 against reference(fp64) under the same rule; the per-launch profile shows exactly the documented launches for each
    combination of stages."""
    import harmonize_suite as HS
    host = HS.inputs("soft", 21, 2, 270, 480)
    params = (0.6, 0.8, 0.5, 0.5, 16.0)
    refs = HS.references_for(*host, params, fast64=True)
    dev = _cuda(*_t(*host))

    def profiled(*p):
        bare_engine.profile(True)
        got = _full(bare_engine)(*dev, *p)
        bare_engine.profile(False)
        res = bare_engine.profile_results()
        assert {k: v["launches"] for k, v in res.items()} == {k: 1 for k in HS.stages_on(p)}, res
        dump = bare_engine.profile_dump()
        assert all(dump.count("\n" + k) == 1 for k in HS.stages_on(p))
        return got
    HS.compare("soft_2x270x480_s16", profiled(*params), refs)
    assert bare_engine.last_forward_ms() > 0.0
    for p in ((0.6, 0.8, 0.5, 0.0, 6.0), (0.0, 0.0, 0.5, 0.5, 0.3), (0.0, 0.0, 0.0, 0.0, 6.0)):
        profiled(*p)


def test_gpu_harmonize_exact_statistics(bare_engine):
    import harmonize_suite as HS
    fg, alpha, bg, params, _, _ = HS.exact_case()
    HS.check_exact(bare_engine.harmonize(*_cuda(*_t(fg, alpha, bg)), *params, return_map=True)[1].cpu().numpy(), "MI355X")


def test_gpu_harmonize_serves_its_purpose(bare_engine):
    """The matched subject has the scene's colour moments; the scene's light wraps the edge that faces it and only that one."""
    import harmonize_suite as HS
    fg, alpha, bg, params = HS.match_scene()
    HS.check_match_purpose(bare_engine.harmonize(*_cuda(*_t(fg, alpha, bg)), *params, return_fg=True)[1].cpu().numpy(), "MI355X")
    fg, alpha, bg, params = HS.wrap_scene()
    HS.check_wrap_purpose(bare_engine.harmonize(*_cuda(*_t(fg, alpha, bg)), *params, return_fg=True)[1].cpu().numpy(), "MI355X")


def test_gpu_harmonize_memory_is_counted_and_released(bare_engine):
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    fg, a, bg = torch.rand(4, 128, 128, 3), torch.rand(4, 128, 128), torch.rand(1, 128, 128, 3)
    px = 4 * 128 * 128
    bare_engine.harmonize(fg, a, bg)
    # host pointers: staging in (3 + 1 floats per pixel, 3 per background pixel) and out (3); T (4 per pixel) and the partials (14 per run) in the arena
    assert bare_engine.resident_bytes() >= bare_engine.weight_bytes() + px * 4 * (4 + 3 + 4) + px // 4 * 12 + 4 * 4 * 56
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    bare_engine.harmonize(fg.cuda(), a.cuda(), bg.cuda())
    assert bare_engine.resident_bytes() >= bare_engine.weight_bytes() + px * 16 + 4 * 4 * 56      # device pointers: the arena alone
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    bare_engine.harmonize(fg.cuda(), a.cuda(), bg.cuda(), wrap_strength=0.0)
    assert bare_engine.weight_bytes() + 4 * 4 * 56 <= bare_engine.resident_bytes() < bare_engine.weight_bytes() + px * 16      # no plane without the wrap
    bare_engine.release_memory()
    with pytest.raises(ValueError):
        bare_engine.harmonize(fg.cuda(), a.cuda(), bg.cuda(), wrap_sigma=16.5)
    with pytest.raises(ValueError):
        bare_engine.harmonize(fg.cuda(), a, bg.cuda())                                # one device for all tensors
    with pytest.raises(ValueError):
        bare_engine.harmonize(fg.cuda(), a.cuda(), bg)
