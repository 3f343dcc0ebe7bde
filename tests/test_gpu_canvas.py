"""The cut-out on a canvas on the MI355X (csrc/k_canvas.h through sdm_compose_canvas): the cases and references of tests/canvas_suite.py.  No weights, small
shapes: the file stays cheap."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def eng(pkg):
    """An engine that never loads weights: sdm_compose_canvas needs none."""
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    e = Engine(SDMatteConfig.tiny(), 0)
    yield e
    e.close()


def test_gpu_canvas_case_list_device_pointers(eng):
    """Every case: placement exact, values within the bound of canvas_suite.py, 5 launches without a shadow and 7 with one."""
    import canvas_suite as CS
    assert len(CS.check_all(eng, lambda t: t.cuda())) == len(CS.cases())


def test_gpu_canvas_host_pointers_give_the_same_bits(eng):
    import canvas_suite as CS
    for case in CS.cases():
        name, fg, alpha, kw = case
        host, ph = CS.check_case(eng, lambda t: t, case)
        dev, pd = eng.compose_canvas(fg.cuda(), alpha.cuda(), return_placement=True, **CS._dev_kw(kw, lambda t: t.cuda()))
        assert torch.equal(host, dev.cpu()) and torch.equal(ph, pd.cpu()), name


def test_gpu_canvas_premultiplication_is_real(eng):
    import canvas_suite as CS
    CS.check_premultiplied(lambda fg, a, **kw: eng.compose_canvas(fg.cuda(), a.cuda(), **kw))


def test_gpu_canvas_shadow_switch_and_transparent_canvas(eng):
    import canvas_suite as CS
    CS.check_shadow_off_is_ignored(eng, lambda t: t.cuda())
    CS.check_transparent_shadow(eng, lambda t: t.cuda())


def test_gpu_canvas_batch_independence_and_launch_counts(eng):
    import canvas_suite as CS
    CS.check_batch_independence(eng, lambda t: t.cuda())
    CS.check_launch_counts_do_not_depend_on_input(eng, lambda t: t.cuda())


def test_gpu_canvas_argument_checks(eng):
    import canvas_suite as CS
    CS.check_errors(eng, lambda t: t.cuda())
    CS.check_errors(eng, lambda t: t)


def test_gpu_canvas_unaligned_output_takes_the_scalar_stores(eng):
    """An output behind a pointer that is not 16-byte aligned: the same bits as the aligned call, 3 and 4 channels, with and without a shadow."""
    import canvas_suite as CS
    import roi_suite as RS
    for nm in ("downscale_b2_rgba", "downscale_b2_colour_rgb", "shadow_leaves_canvas_colour", "shadow_transparent"):
        name, fg, alpha, kw = next(c for c in CS.cases() if c[0] == nm)
        base = eng.compose_canvas(fg.cuda(), alpha.cuda(), **kw)
        out = RS.misaligned(torch.empty_like(base))
        assert eng.compose_canvas(fg.cuda(), alpha.cuda(), out=out, **kw) is out
        assert torch.equal(out, base), nm


def test_gpu_canvas_on_a_side_stream(eng):
    """Inputs produced on a side stream right before the call, the canvas consumed on it right after: the engine orders itself on both ends."""
    import canvas_suite as CS
    name, fg, alpha, kw = next(c for c in CS.cases() if c[0] == "shadow_leaves_canvas_colour")
    want = eng.compose_canvas(fg.cuda(), (alpha * 0.5).cuda(), **kw) * 2
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        half = alpha.cuda() * 0.5
        doubled = eng.compose_canvas(fg.cuda(), half, sync=False, **kw) * 2
    st.synchronize()
    assert torch.equal(doubled, want)


def test_gpu_canvas_memory_is_counted_and_released(eng):
    eng.release_memory()
    assert eng.resident_bytes() == eng.weight_bytes()
    fg, a = torch.rand(1, 24, 20, 3), torch.rand(1, 24, 20)
    eng.compose_canvas(fg.cuda(), a.cuda(), 32, 48)
    plain = eng.resident_bytes()
    assert plain > eng.weight_bytes()                                        # raw extrema, box, placements (arena)
    eng.compose_canvas(fg.cuda(), a.cuda(), 32, 48, shadow_opacity=0.5, shadow_sigma=2.0)
    shadow = eng.resident_bytes()
    assert shadow >= plain + 32 * 48 * 20                                    # the layer (16 bytes per canvas pixel) and the blur plane (4)
    eng.compose_canvas(fg, a, 32, 48)
    assert eng.resident_bytes() >= shadow + 24 * 20 * 16 + 32 * 48 * 16      # host pointers: staging in and out
    eng.release_memory()
    assert eng.resident_bytes() == eng.weight_bytes()


def test_gpu_canvas_profile_shows_each_launch_once(eng):
    import canvas_suite as CS
    for shadow, want in ((0.0, CS.PLAIN_KERNELS), (0.5, CS.SHADOW_KERNELS)):
        eng.profile(True)
        eng.compose_canvas(torch.rand(2, 37, 53, 3).cuda(), torch.rand(2, 37, 53).cuda(), 32, 48, shadow_opacity=shadow, shadow_sigma=2.0)
        eng.profile(False)
        res = eng.profile_results()
        assert {k: res[k]["launches"] for k in res} == {k: 1 for k in want}, sorted(res)
        assert eng.last_forward_ms() > 0.0
