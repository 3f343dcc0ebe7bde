"""Green-screen calls on the MI355X (csrc/k_key.h through sdm_screen_colour and sdm_chroma_key) against the numpy reference of tests/key_suite.py under
its rules: integers, key, trimap and despilled bit for bit, the colour within max(4 d32, 2^-20).  No weights, no oracle forward: the file stays cheap
(durations in profiles/NOTES.md)."""
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
    """An engine that never loads weights: the key calls need none."""
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)
    yield eng
    eng.close()


def _nosync(fn):
    return lambda *a, **kw: fn(*a, sync=False, **kw)


def test_gpu_key_case_list_device_pointers(bare_engine):
    """Device tensors on torch's current stream (sync=False: the results are read through that stream, as the stream contract promises); the launch
    counts of the whole run are the documented ones per call."""
    import key_suite as KS
    e = bare_engine
    e.lib.kernel_counts(reset=True)
    n = KS.check_colour(_nosync(e.screen_colour), lambda t: t.cuda())
    assert e.lib.kernel_counts() == {k: n for k in KS.COLOUR_LAUNCHES}
    e.lib.kernel_counts(reset=True)
    plan = KS.check_key(_nosync(e.chroma_key), lambda t: t.cuda())
    assert e.lib.kernel_counts() == KS.key_launches(plan)


def test_gpu_key_case_list_host_pointers(bare_engine):
    import key_suite as KS
    KS.check_colour(bare_engine.screen_colour, lambda t: t)
    KS.check_key(bare_engine.chroma_key, lambda t: t)


def test_gpu_key_on_a_side_stream(bare_engine):
    """The inputs are produced on a side stream right before the calls and the results consumed on it right after: the engine orders itself on both
    ends, and the two calls on each other."""
    import key_suite as KS
    img = KS.inputs("screen", 3, 2, 150, 260)
    half = (img * np.float32(0.5)).astype(np.float32)                   # (exact: the values are multiples of 2^-10)
    c64, info_ref = KS.colour_reference(half, 1, 0)
    base = torch.from_numpy(img).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        x = base * 0.5
        colour, info = bare_engine.screen_colour(x, "green", return_info=True, sync=False)
        key, tri, desp = bare_engine.chroma_key(x, colour, erode_px=4, dilate_px=6, sync=False)
        outs = [t * 1.0 for t in (colour, key, tri, desp)]
    st.synchronize()
    assert np.array_equal(info.cpu().numpy(), info_ref) and float(np.abs(outs[0].cpu().numpy() - c64).max()) <= 2.0 ** -20
    ref = KS.key_reference(half, outs[0].cpu().numpy(), KS.DEFAULTS[:4] + (4, 6, 1.0))
    assert all(KS.same_bits(g, ref[w]) for g, w in zip(outs[1:], KS.OUTPUTS))


@pytest.mark.parametrize("H,W", [(130, 260), (64, 256), (9, 37)])
def test_gpu_key_is_deterministic(bare_engine, H, W):
    """Identity 6: two calls are bit-identical; device pointers and host pointers give the same bits; a batch equals per-image calls; tensors 4 bytes off
    a 16-byte boundary (the scalar paths) give the bits of the aligned ones."""
    import key_suite as KS
    e = bare_engine
    img = torch.from_numpy(KS.inputs("dirty", 7, 3, H, W))
    plane = torch.from_numpy(KS.inputs("screen", 8, 3, H, W))
    d_img, d_plane = img.cuda(), plane.cuda()
    colour, info = e.screen_colour(d_img, "any", return_info=True)
    shared = e.screen_colour(d_img, "any", share=True)
    outs = e.chroma_key(d_img, d_plane, erode_px=3, dilate_px=5)
    same = lambda a, b: all(KS.same_bits(x, y) for x, y in zip(a, b))
    assert same(outs, e.chroma_key(d_img, d_plane, erode_px=3, dilate_px=5))
    c2, i2 = e.screen_colour(d_img, "any", return_info=True)
    assert KS.same_bits(colour, c2) and torch.equal(info, i2)
    h = e.chroma_key(img, plane, erode_px=3, dilate_px=5)
    assert all(t.device.type == "cpu" for t in h) and same(outs, h)
    hc, hi = e.screen_colour(img, "any", return_info=True)
    assert KS.same_bits(colour, hc) and torch.equal(info.cpu(), hi) and KS.same_bits(shared, e.screen_colour(img, "any", share=True))
    for b in range(3):
        one = e.chroma_key(d_img[b:b + 1].contiguous(), d_plane[b:b + 1].contiguous(), erode_px=3, dilate_px=5)
        assert same([t[b:b + 1] for t in outs], one), b
        assert KS.same_bits(colour[b:b + 1], e.screen_colour(d_img[b:b + 1].contiguous(), "any")), b
    offs = []
    for t in (d_img, d_plane):
        buf = torch.empty(t.numel() + 1, device="cuda")
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert t.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 and v.is_contiguous()
        offs.append(v)
    assert same(outs, e.chroma_key(*offs, erode_px=3, dilate_px=5)) and same(outs, e.chroma_key(d_img, offs[1], erode_px=3, dilate_px=5))
    c3, i3 = e.screen_colour(offs[0], "any", return_info=True)
    assert KS.same_bits(colour, c3) and torch.equal(info, i3) and KS.same_bits(shared, e.screen_colour(offs[0], "any", share=True))


def test_gpu_key_identities(bare_engine):
    """The seven identities of the header on device tensors, identity 5 against the existing sdm_make_trimap."""
    import key_suite as KS
    KS.check_identities(bare_engine.screen_colour, bare_engine.chroma_key, lambda t: t.cuda(), "MI355X")
    KS.check_trimap_formula(bare_engine.chroma_key, bare_engine.make_trimap, lambda t: t.cuda(), "MI355X")


def test_gpu_key_2x270x480_and_launch_counts(bare_engine):
    """2 x 270 x 480 under the same rules; the per-launch profile shows exactly the documented launches of each call."""
    import key_suite as KS
    e = bare_engine
    img = KS.inputs("screen", 21, 2, 270, 480)
    d_img = torch.from_numpy(img).cuda()

    def profiled(launches, fn, *args, **kw):
        e.profile(True)
        out = fn(*args, **kw)
        e.profile(False)
        res = e.profile_results()
        assert {k: v["launches"] for k, v in res.items()} == launches, res
        dump = e.profile_dump()
        assert all(dump.count("\n" + k) == n for k, n in launches.items())
        return out
    for share in (False, True):
        refs = [KS.colour_reference(img, 1, int(share), v) for v in ("f64", "runs32", "rows32")]
        d32 = max(float(np.abs(r[0] - refs[0][0]).max()) for r in refs[1:])
        colour, info = profiled(e.SCREEN_COLOUR_LAUNCHES, e.screen_colour, d_img, "green", share, return_info=True)
        assert np.array_equal(info.cpu().numpy(), refs[0][1])
        d = float(np.abs(colour.cpu().numpy().astype(np.float64) - refs[0][0]).max())
        print(f"[key] 2x270x480 share={share} colour: d32 = {d32:.3e} tol = {KS.tolerance(d32):.3e} d = {d:.3e}")
        assert d <= KS.tolerance(d32)
    assert e.last_forward_ms() > 0.0
    ref = KS.key_reference(img, colour.cpu().numpy(), KS.DEFAULTS)
    outs = profiled(e.key_launches(KS.OUTPUTS), e.chroma_key, d_img, colour)
    assert all(KS.same_bits(g, ref[w]) for g, w in zip(outs, KS.OUTPUTS))
    desp = profiled({"ck_key": 1}, e.chroma_key, d_img, colour, want="despilled")
    assert KS.same_bits(desp, ref["despilled"])


def test_gpu_key_serves_its_purpose(bare_engine):
    """No definite pixel of the trimap is wrong, the second pass shrinks the unknown band and the key error, the despilled image carries no green excess;
    Engine.key_screen is the chain, bit for bit."""
    import key_suite as KS
    e = bare_engine
    KS.check_purpose(e.screen_colour, e.chroma_key, e.fill_background, lambda t: t.cuda(), "MI355X", e.key_screen)


def test_gpu_key_memory_is_counted_and_released(bare_engine):
    e = bare_engine
    e.release_memory()
    assert e.resident_bytes() == e.weight_bytes()
    img = torch.rand(4, 128, 128, 3).cuda()
    colour = e.screen_colour(img, "any")
    # device pointers: the arena alone - a histogram slot per image, {eligible, mode} and 4 runs of partials per image
    assert e.resident_bytes() >= e.weight_bytes() + 4 * 4096 * 4 + 4 * 4 * 16
    e.release_memory()
    assert e.resident_bytes() == e.weight_bytes()
    e.chroma_key(img, colour, want=("key", "despilled"))
    assert e.resident_bytes() == e.weight_bytes()                        # one pointwise launch: nothing in the arena
    e.chroma_key(img, colour)
    assert e.resident_bytes() >= e.weight_bytes() + 4 * 128 * 128 * (1 + 2)      # the class bytes and the int16 plane
    e.release_memory()
    e.chroma_key(img, colour, want="trimap")
    assert e.resident_bytes() >= e.weight_bytes() + 4 * 128 * 128 * (1 + 2 + 4)  # ... and the key, when it is not an output
    e.release_memory()
    assert e.resident_bytes() == e.weight_bytes()
    with pytest.raises(ValueError):
        e.chroma_key(img, colour.cpu())                                  # one device for all tensors
    with pytest.raises(ValueError):
        e.chroma_key(img, colour, clip_bg=0.1)
    with pytest.raises(ValueError):
        e.screen_colour(img, "red")
