"""The subject's box and the cropped node call on the kernel emulator: the kernels of csrc/k_roi.h (both load paths, the wave and block reduction, the
atomics, the integer box) against the brute force, and sdm_apply_matte_roi against the composition of existing calls on the tiny architecture.
The real-kernel versions are tests/test_gpu_roi.py."""
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
def loaded_engine(pkg):
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.weights import synthetic_state_dict
    cfg = SDMatteConfig.tiny()
    eng = _emu_engine(cfg)
    eng.load_state_dict(synthetic_state_dict(cfg, 0))
    yield eng
    eng.close()


def test_emu_subject_roi_case_list(pkg):
    """Every case of the list on an engine that never loaded weights: equal to the brute force and the CPU restatement, three launches each."""
    import roi_suite as RS
    eng = _emu_engine()
    RS.check_subject_roi(eng, lambda t: t)
    eng.close()


def test_emu_subject_roi_unaligned_pointer_takes_the_scalar_path(pkg):
    """96 x 128 behind a pointer that is not 16-byte aligned, B = 1 and B = 3: the same boxes as the aligned tensor."""
    import roi_suite as RS
    eng = _emu_engine()
    cases = [c for c in RS.box_cases() if c[0] in ("vector_path_96x128", "soft_threshold_0.3_square_96x128", "vector_path_blocks_300x516")]
    assert len(cases) == 3
    RS.check_subject_roi(eng, RS.misaligned, cases)
    three = torch.from_numpy(RS.rect(96, 128, 10, 40, 8, 100, B=3))
    three[1] = three[1].roll((30, 9), (0, 1))
    three[2, :, 50:] = 0.0
    assert torch.equal(eng.subject_roi(RS.misaligned(three)), eng.subject_roi(three))
    eng.close()


def test_emu_subject_roi_argument_checks_and_memory(pkg):
    """Out-of-range arguments raise (Python check and SDM_ERR_INVALID of the C ABI, output untouched); no SDM_ERR_STATE without weights; what the call
    keeps is counted by resident_bytes and given back by release_memory."""
    import roi_suite as RS
    eng = _emu_engine()
    RS.check_subject_roi_errors(eng, lambda t: t)
    eng.release_memory()
    assert eng.resident_bytes() == eng.weight_bytes()
    eng.subject_roi(torch.rand(1, 20, 30))
    assert eng.resident_bytes() > eng.weight_bytes()                     # the raw extrema (arena)
    eng.release_memory()
    assert eng.resident_bytes() == eng.weight_bytes()
    eng.subject_roi(torch.rand(1, 20, 30))                               # ... and the next call allocates again
    eng.close()


def test_emu_apply_matte_roi_equals_composition(loaded_engine):
    """Tiny architecture, image 96 x 128 at inference size 64: alpha, matted and roi equal box + crop + apply_matte_node + paste + tail for every output
    mode with mask_refine on and off; each roi_ kernel runs once per call; no SDM_ERR_ARENA."""
    import roi_suite as RS
    RS.check_roi_call_equals_composition(loaded_engine, lambda t: t)


def test_emu_apply_matte_roi_batch_of_two(loaded_engine):
    """Two boxes of one size at different offsets against ONE B = 2 reference call."""
    import roi_suite as RS
    RS.check_roi_call_equals_composition(loaded_engine, lambda t: t, modes=("matted_rgb", ), refines=(True, ), rects=((10, 50, 20, 70), (30, 70, 50, 100)))


def test_emu_apply_matte_roi_from_mask_copy_shortcut_and_empty(loaded_engine):
    import roi_suite as RS
    RS.check_roi_call_from_mask(loaded_engine, lambda t: t)
    RS.check_roi_call_copy_shortcut(loaded_engine, lambda t: t)
    RS.check_roi_call_empty(loaded_engine, lambda t: t)


def test_emu_apply_matte_roi_independence_and_errors(loaded_engine):
    import roi_suite as RS
    RS.check_roi_call_independent_of_outside(loaded_engine, lambda t: t)
    RS.check_roi_call_errors(loaded_engine, lambda t: t)


def test_emu_fan_out_apply_matte_roi(pkg):
    """MultiGpuEngine.apply_matte_roi splits the batch like apply_matte_mask: the same bits as one engine fed the same shards; subject_roi runs on the
    first engine."""
    import roi_suite as RS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.parallel import MultiGpuEngine
    from comfyui_sdmatte_amd.weights import synthetic_state_dict
    cfg = SDMatteConfig.tiny()
    w = synthetic_state_dict(cfg, 0)
    one = _emu_engine(cfg)
    one.load_state_dict(w)
    fan = MultiGpuEngine(cfg, [0, 1], _engine_factory=lambda d: _emu_engine(cfg))
    fan.load_state_dict(w)
    image, mask = RS.e2e_inputs(((20, 60, 30, 90), (5, 80, 60, 120)), seed=11)
    args = (64, False, "matted_rgba", True, 0.8, True, 0.4, 2, 3, 0.0, 3, 5, False)
    fa, fm, ft, fr = fan.apply_matte_roi(image, mask, *args)
    assert fr.dtype == torch.int32 and fr[0].tolist() != fr[1].tolist()
    for i in range(2):
        a, m, t, r = one.apply_matte_roi(image[i:i + 1], mask[i:i + 1], *args)
        assert torch.equal(fa[i:i + 1], a) and torch.equal(fm[i:i + 1], m) and torch.equal(ft[i:i + 1], t) and torch.equal(fr[i:i + 1], r)
    assert torch.equal(fan.subject_roi(ft, 0.0, 3, 5, False), fr)
    fa2, fm2, ft2, fr2 = fan.apply_matte_roi(image, ft, 64, False, "alpha_only", False, 0.8, margin_px=3, margin_pct=5, square=False)
    assert ft2 is None and torch.equal(fr2, fr) and fm2.shape[-1] == 3
    one.close(); fan.close()
