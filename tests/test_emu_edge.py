"""The distance field and its two consumers on the kernel emulator: the kernels of csrc/k_distance.h (the tile words, the carries across tiles, the
chunk pruning of the row search, the fused consumers) against the references of tests/edge_suite.py.  The real-kernel versions, with the large sizes,
are tests/test_gpu_edge.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _emu_engine(cfg=None):
    from emu.build_emu import build
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Bindings, Engine
    return Engine(cfg or SDMatteConfig.tiny(), 0, True, _lib=Bindings(ctypes.CDLL(build())), precision="fp16")


@pytest.fixture(scope="module")
def bare_engine(pkg):
    """An engine that never loads weights: the three calls need none."""
    eng = _emu_engine()
    yield eng
    eng.close()


def test_emu_distance_field_equals_brute_force(bare_engine):
    import edge_suite as ES
    ES.check_field(bare_engine, lambda t: t, ES.field_cases("brute"))


def test_emu_distance_field_equals_restatement(bare_engine):
    """Every content at every size of the list: one pixel, single rows and columns, more than one chunk, tile and segment, 79 tiles, 40 chunks."""
    import edge_suite as ES
    ES.check_field(bare_engine, lambda t: t, ES.field_cases("restatement"))


def test_emu_distance_field_batch_and_misaligned_pointer(bare_engine):
    import edge_suite as ES
    import roi_suite as RS
    ES.check_field_batch(bare_engine, lambda t: t)
    ES.check_field_batch(bare_engine, RS.misaligned)


def test_emu_distance_field_seeds_and_long_row(bare_engine):
    """The closed forms at a size the emulator affords (12 seeds at 100 x 180, B = 2), their complement, and one seed in a row of 32768."""
    import edge_suite as ES
    plane, field = ES.seed_case(100, 180, 12)
    assert int((field == 1).sum()) >= 8 and int((field == 2).sum()) >= 2      # isolated seeds, and the centre of a clump in either image
    assert np.array_equal(bare_engine.distance_field(torch.from_numpy(plane)).numpy(), field)
    assert np.array_equal(bare_engine.distance_field(torch.from_numpy(1.0 - plane)).numpy(), -field)
    plane, field = ES.long_row_case()
    assert np.array_equal(bare_engine.distance_field(torch.from_numpy(plane)).numpy(), field)


def test_emu_distance_field_against_trimap_kernels(bare_engine):
    import edge_suite as ES
    ES.check_field_against_trimap(bare_engine, lambda t: t, 97, 131, ((0, 0), (1, 2), (10, 10), (255, 255)))


def test_emu_offset_mask(bare_engine):
    import edge_suite as ES
    ES.check_offset_mask(bare_engine, lambda t: t)
    ES.check_offset_mask_exact_consequences(bare_engine, lambda t: t)


def test_emu_outline(bare_engine):
    import edge_suite as ES
    ES.check_outline(bare_engine, lambda t: t)
    ES.check_outline_exact_properties(bare_engine, lambda t: t)


def test_emu_edge_argument_checks_and_memory(bare_engine):
    import edge_suite as ES
    ES.check_errors(bare_engine, lambda t: t)
    ES.check_memory(bare_engine, lambda t: t)


def test_emu_fan_out_edge_calls(pkg):
    """MultiGpuEngine runs the three calls on its first engine, results on the host: the same bits as one engine."""
    import edge_suite as ES
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.parallel import MultiGpuEngine
    cfg = SDMatteConfig.tiny()
    one = _emu_engine(cfg)
    fan = MultiGpuEngine(cfg, [0, 1], _engine_factory=lambda d: _emu_engine(cfg))
    fg, alpha = ES.outline_inputs(45, 70)
    assert torch.equal(fan.distance_field(alpha, 0.3), one.distance_field(alpha, 0.3))
    assert torch.equal(fan.offset_mask(alpha, 4.5, 3.0, 0.3), one.offset_mask(alpha, 4.5, 3.0, 0.3))
    got, want = fan.outline(fg, alpha, 5.5, (0.2, 0.4, 0.6), "center", 2.0, 0.9, 0.3), one.outline(fg, alpha, 5.5, (0.2, 0.4, 0.6), "center", 2.0, 0.9, 0.3)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[0].device.type == "cpu"
    one.close(); fan.close()
