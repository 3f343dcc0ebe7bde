"""A box per subject and the node call over a list of boxes on the kernel emulator: the kernels of csrc/k_boxes.h (the rank launches, both load paths of the
two reductions, the containment rule, the rest box, the sanitised list, the maximum paste) against the brute force and the compositions of
tests/boxes_suite.py.  The real-kernel versions are tests/test_gpu_boxes.py."""
import ctypes
import os
import sys

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


def test_emu_subject_boxes_case_list(bare_engine):
    """Every case of the list on an engine that never loaded weights: equal to the brute force and the CPU restatement, 8 + 2 (max_boxes - 1) launches."""
    import boxes_suite as BS
    BS.check_subject_boxes(bare_engine, lambda t: t)


def test_emu_subject_boxes_unaligned_pointer(bare_engine):
    """96 x 128 behind a pointer that is not 16-byte aligned: the same boxes."""
    import boxes_suite as BS
    import roi_suite as RS
    cases = [c for c in BS.box_cases() if c[0].startswith("vector_path_96x128")]
    assert len(cases) == 2
    BS.check_subject_boxes(bare_engine, RS.misaligned, cases)


def test_emu_subject_boxes_launches_depend_on_max_boxes_only(bare_engine):
    import boxes_suite as BS
    for K in (1, 2, 5, 8):
        seen = []
        for plane in (torch.zeros(1, 40, 50), torch.rand(2, 70, 130), torch.ones(1, 3, 200)):
            bare_engine.lib.kernel_counts(reset=True)
            bare_engine.subject_boxes(plane, 0.5, 2, K)
            seen.append(bare_engine.lib.kernel_counts())
        assert seen[0] == seen[1] == seen[2] == BS.launches(K) and sum(seen[0].values()) == 8 + 2 * (K - 1)


def test_emu_subject_boxes_argument_checks_and_memory(bare_engine):
    import boxes_suite as BS
    BS.check_subject_boxes_errors(bare_engine, lambda t: t)
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    bare_engine.subject_boxes(torch.rand(1, 20, 30))
    assert bare_engine.resident_bytes() >= bare_engine.weight_bytes() + 3 * 20 * 30 * 4      # the three label planes (arena)
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    bare_engine.subject_boxes(torch.rand(1, 20, 30))                                          # ... and the next call allocates again


def test_emu_apply_matte_boxes_equals_roi_call(loaded_engine):
    import boxes_suite as BS
    BS.check_equals_roi_call(loaded_engine, lambda t: t)


def test_emu_apply_matte_boxes_equals_composition(loaded_engine):
    """Two disjoint boxes and two overlapping ones in one image; B = 2 with three entries in mixed image order; a box of exactly S x S."""
    import boxes_suite as BS
    BS.check_equals_composition(loaded_engine, lambda t: t, [[0, 5, 8, 40, 48], [0, 50, 70, 40, 48]], modes=(("matted_rgb", True), ))
    BS.check_equals_composition(loaded_engine, lambda t: t, [[0, 10, 20, 48, 56], [0, 30, 50, 48, 56]], overlap=(30, 58, 50, 76))
    BS.check_equals_composition(loaded_engine, lambda t: t, [[1, 20, 60, 44, 44], [0, 8, 8, 44, 44], [1, 40, 10, 44, 44]], B=2, modes=(("matted_rgba", False), ))
    BS.check_equals_composition(loaded_engine, lambda t: t, [[0, 16, 32, 64, 64]])


def test_emu_apply_matte_boxes_void_entries_and_errors(loaded_engine):
    import boxes_suite as BS
    BS.check_void_entries(loaded_engine, lambda t: t)
    BS.check_call_errors(loaded_engine, lambda t: t)


def test_emu_fan_out_apply_matte_boxes(pkg):
    """MultiGpuEngine.apply_matte_boxes shards by image and rebases b: the bits of one engine fed the same shards; an image without an entry gets alpha 0;
    subject_boxes runs on the first engine."""
    import boxes_suite as BS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.parallel import MultiGpuEngine
    from comfyui_sdmatte_amd.weights import synthetic_state_dict
    cfg = SDMatteConfig.tiny()
    w = synthetic_state_dict(cfg, 0)
    one = _emu_engine(cfg)
    one.load_state_dict(w)
    fan = MultiGpuEngine(cfg, [0, 1], _engine_factory=lambda d: _emu_engine(cfg))
    fan.load_state_dict(w)
    image, trimap = BS.frames(2, seed=31)
    boxes = BS.boxes_tensor([[1, 20, 60, 44, 50], [0, 8, 8, 40, 40], [1, 40, 10, 30, 60]])
    fa, fm = fan.apply_matte_boxes(image, trimap, boxes, 64, False, "matted_rgba", True, 0.8)
    for i, part in ((0, [[0, 8, 8, 40, 40]]), (1, [[0, 20, 60, 44, 50], [0, 40, 10, 30, 60]])):
        assert fan.shard_boxes(boxes, i, i + 1).tolist() == part
        a, m = one.apply_matte_boxes(image[i:i + 1], trimap[i:i + 1], BS.boxes_tensor(part), 64, False, "matted_rgba", True, 0.8)
        assert torch.equal(fa[i:i + 1], a) and torch.equal(fm[i:i + 1], m)
    fa, _ = fan.apply_matte_boxes(image, trimap, boxes[:1], 64, False, "alpha_only", False, 0.8)
    assert fan.shard_boxes(boxes[:1], 0, 1).tolist() == [BS.VOID] and bool((fa[0] == 0.0).all()) and float(fa[1].max()) > 0.0
    plane = torch.from_numpy(BS.paint(97, 131, BS.THREE))
    assert torch.equal(fan.subject_boxes(plane, 0.0, 64, 3, 2, 5, False), one.subject_boxes(plane, 0.0, 64, 3, 2, 5, False))
    one.close(); fan.close()
