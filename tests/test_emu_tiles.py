"""Tiles along the unknown band and the node call that blends them on the kernel emulator: the kernels of csrc/k_tiles.h (both load paths of the mark
kernel, the ranges from the origin tables, the ordered list, the culled weighted blend) against the brute force and the compositions of
tests/tiles_suite.py, with host pointers.  The real-kernel versions are tests/test_gpu_tiles.py."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
EMU_MODES = (("alpha_only", False), ("matted_rgba", True), ("matted_rgb", True))


def _emu_engine(cfg=None):
    from emu.build_emu import build
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Bindings, Engine
    return Engine(cfg or SDMatteConfig.tiny(), 0, True, _lib=Bindings(ctypes.CDLL(build())), precision="fp16")


@pytest.fixture(scope="module")
def bare_engine(pkg):
    eng = _emu_engine()
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def loaded_engine(pkg):
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.weights import synthetic_state_dict
    cfg = SDMatteConfig.tiny()
    eng = _emu_engine(cfg)
    eng.load_state_dict(synthetic_state_dict(cfg, 0))
    yield eng
    eng.close()


def test_emu_band_tiles_case_list(bare_engine):
    """Every case of the list on an engine that never loaded weights: equal to the brute force and the CPU restatement, three launches each."""
    import tiles_suite as TS
    TS.check_cases_mean_what_their_names_say()
    TS.check_band_tiles(bare_engine, lambda t: t)


def test_emu_band_tiles_unaligned_pointer(bare_engine):
    """96 x 128 behind a pointer that is not 16-byte aligned (the scalar path on a shape of the vector path): the same tiles."""
    import roi_suite as RS
    import tiles_suite as TS
    cases = [c for c in TS.band_cases() if c[0].startswith("ring_96x128")]
    assert len(cases) == 5
    TS.check_band_tiles(bare_engine, RS.misaligned, cases)


def test_emu_band_tiles_launches_depend_on_nothing(bare_engine):
    import tiles_suite as TS
    for plane, T, O in ((torch.zeros(1, 40, 50), 64, 16), (torch.rand(2, 70, 130), 16, 8), (torch.full((1, 3, 200), 0.5), 32, 0)):
        bare_engine.lib.kernel_counts(reset=True)
        bare_engine.band_tiles(plane, tile=T, overlap=O)
        assert bare_engine.lib.kernel_counts() == {k: 1 for k in TS.BAND_KERNELS}


def test_emu_band_tiles_argument_checks_and_memory(bare_engine):
    import tiles_suite as TS
    TS.check_band_tiles_errors(bare_engine, lambda t: t)
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    bare_engine.band_tiles(torch.rand(1, 20, 30))
    assert bare_engine.resident_bytes() >= bare_engine.weight_bytes() + 8 * 4                         # the flag words of one image (arena)
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    bare_engine.band_tiles(torch.rand(1, 20, 30))                                                      # ... and the next call allocates again


def test_emu_apply_matte_tiles_equals_node_call(loaded_engine):
    """One tile = the frame, every output mode, mask_refine on and off among them (a model pass takes seconds here: the GPU file runs all six)."""
    import tiles_suite as TS
    TS.check_equals_node_call(loaded_engine, lambda t: t, EMU_MODES)


def test_emu_apply_matte_tiles_disjoint_tiles_are_exact(loaded_engine):
    import tiles_suite as TS
    TS.check_disjoint_tiles(loaded_engine, lambda t: t, EMU_MODES)


def test_emu_apply_matte_tiles_overlapping_tiles(loaded_engine):
    import tiles_suite as TS
    TS.check_overlapping_tiles(loaded_engine, lambda t: t, modes80=TS.MODES_OV[1:])


def test_emu_apply_matte_tiles_mixed_order_and_base(loaded_engine):
    import tiles_suite as TS
    TS.check_mixed_order_and_base(loaded_engine, lambda t: t, modes=TS.MODES_OV[1:], modes_base=TS.MODES_OV[:1])


def test_emu_apply_matte_tiles_structure(loaded_engine):
    """Equal slot values, N = 0, void entries among valid ones."""
    import tiles_suite as TS
    TS.check_constant_slots(loaded_engine, lambda t: t)
    TS.check_no_tiles(loaded_engine, lambda t: t)
    TS.check_void_entries(loaded_engine, lambda t: t)


def test_emu_apply_matte_tiles_errors(loaded_engine):
    import tiles_suite as TS
    TS.check_call_errors(loaded_engine, lambda t: t)
