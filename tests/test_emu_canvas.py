"""The cut-out on a canvas on the kernel emulator: the kernels of csrc/k_canvas.h (the fit, the fused place-and-compose launch, the place / row blur /
column-blur-and-compose launches of the shadow) through sdm_compose_canvas, against the cases and references of tests/canvas_suite.py.  The real-kernel
versions are tests/test_gpu_canvas.py."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def eng(pkg):
    """An engine that never loads weights: sdm_compose_canvas needs none."""
    from emu.build_emu import build
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Bindings, Engine
    e = Engine(SDMatteConfig.tiny(), 0, True, _lib=Bindings(ctypes.CDLL(build())), precision="fp16")
    yield e
    e.close()


def test_emu_canvas_case_list_without_shadow(eng):
    """Placement exact, values within the bound, five launches, no SDM_ERR_ARENA (it would raise): every case without a shadow."""
    import canvas_suite as CS
    names = CS.check_all(eng, lambda t: t, lambda n: "shadow" not in n)
    assert len(names) >= 20 and {"copy_branch", "empty_alpha", "nan_alpha", "edge_box", "upscale_fill100"} <= set(names)


def test_emu_canvas_case_list_with_shadow(eng):
    """The same with a shadow (seven launches): part of it beyond the canvas, a radius larger than canvas and tile, a transparent canvas, two tiles."""
    import canvas_suite as CS
    names = CS.check_all(eng, lambda t: t, lambda n: "shadow" in n)
    assert len(names) == 6


def test_emu_canvas_premultiplication_is_real(eng):
    import canvas_suite as CS
    CS.check_premultiplied(eng.compose_canvas)


def test_emu_canvas_shadow_switch_and_transparent_canvas(eng):
    import canvas_suite as CS
    CS.check_shadow_off_is_ignored(eng, lambda t: t)
    CS.check_transparent_shadow(eng, lambda t: t)


def test_emu_canvas_batch_independence_and_launch_counts(eng):
    import canvas_suite as CS
    CS.check_batch_independence(eng, lambda t: t)
    CS.check_launch_counts_do_not_depend_on_input(eng, lambda t: t)


def test_emu_canvas_argument_checks_and_memory(eng):
    """Every invalid argument is refused with nothing written; what the call keeps is counted by resident_bytes and given back by release_memory."""
    import canvas_suite as CS
    CS.check_errors(eng, lambda t: t)
    eng.release_memory()
    assert eng.resident_bytes() == eng.weight_bytes()
    fg, a = torch.rand(1, 24, 20, 3), torch.rand(1, 24, 20)
    eng.compose_canvas(fg, a, 32, 48)
    plain = eng.resident_bytes()
    assert plain > eng.weight_bytes()
    eng.compose_canvas(fg, a, 32, 48, shadow_opacity=0.5, shadow_sigma=2.0)
    assert eng.resident_bytes() >= plain + 32 * 48 * 20                      # the layer (16 bytes per canvas pixel) and the blur plane (4)
    eng.release_memory()
    assert eng.resident_bytes() == eng.weight_bytes()
    eng.compose_canvas(fg, a, 32, 48)                                        # ... and the next call allocates again


def test_emu_fan_out_compose_canvas(pkg):
    """MultiGpuEngine.compose_canvas runs on the first engine and returns what that engine returns."""
    import canvas_suite as CS
    from emu.build_emu import build
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Bindings, Engine
    from comfyui_sdmatte_amd.parallel import MultiGpuEngine
    cfg = SDMatteConfig.tiny()
    make = lambda d: Engine(cfg, 0, True, _lib=Bindings(ctypes.CDLL(build())), precision="fp16")      # noqa: E731
    fan = MultiGpuEngine(cfg, [0, 1], _engine_factory=make)
    name, fg, alpha, kw = next(c for c in CS.cases() if c[0] == "shadow_leaves_canvas_colour")
    out, place = fan.compose_canvas(fg, alpha, return_placement=True, **kw)
    one, p1 = fan.engines[0].compose_canvas(fg, alpha, return_placement=True, **kw)
    assert torch.equal(out, one) and torch.equal(place, p1)
    fan.close()
