"""The subject's box and the cropped node call on the MI355X (csrc/k_roi.h through sdm_subject_roi / sdm_apply_matte_roi): exact against the references of
tests/roi_suite.py.  Tiny architecture only, no oracle forward: the file stays cheap."""
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
    """An engine that never loads weights: sdm_subject_roi needs none."""
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def loaded_engine(pkg):
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.weights import synthetic_state_dict
    cfg = SDMatteConfig.tiny()
    eng = Engine(cfg, 0)
    eng.load_state_dict(synthetic_state_dict(cfg, 0))
    yield eng
    eng.close()


def test_gpu_subject_roi_case_list_device_pointers(bare_engine):
    """Device tensors on torch's current stream (sync=False is exercised by the side-stream test; here the result is read after a sync)."""
    import roi_suite as RS
    RS.check_subject_roi(bare_engine, lambda t: t.cuda())


def test_gpu_subject_roi_case_list_host_pointers(bare_engine):
    import roi_suite as RS
    RS.check_subject_roi(bare_engine, lambda t: t)


def test_gpu_subject_roi_unaligned_device_pointer(bare_engine):
    """96 x 128 (and 300 x 516) on a device tensor sliced so that its pointer is not 16-byte aligned: the scalar path, the same boxes."""
    import roi_suite as RS
    cases = [c for c in RS.box_cases() if c[0] in ("vector_path_96x128", "soft_threshold_0.3_square_96x128", "vector_path_blocks_300x516")]
    assert len(cases) == 3
    RS.check_subject_roi(bare_engine, lambda t: RS.misaligned(t.cuda()), cases)
    three = torch.from_numpy(RS.rect(96, 128, 10, 40, 8, 100, B=3))
    three[1] = three[1].roll((30, 9), (0, 1))
    three[2, :, 50:] = 0.0
    want = RS.brute_force(three.numpy(), 0.0, 16, 10, True)
    assert np.array_equal(bare_engine.subject_roi(RS.misaligned(three.cuda())).cpu().numpy(), want)
    assert np.array_equal(bare_engine.subject_roi(three.cuda()).cpu().numpy(), want)


def test_gpu_subject_roi_many_blocks_per_image(bare_engine):
    """1080 x 1920, B = 2: 127 blocks per image meet in the four atomics; a subject in the middle, one pixel in the last row of the second image."""
    import roi_suite as RS
    import trimap_suite as TS
    plane = TS.blobs(41, 2, 1080, 1920, n=3)
    plane[plane < 0.5] = 0.0
    plane[1, 1079, 1919] = 0.25
    for thr in (0.0, 0.3):
        got = bare_engine.subject_roi(torch.from_numpy(plane).cuda(), thr, 16, 10, False).cpu().numpy()
        assert np.array_equal(got, RS.brute_force(plane, thr, 16, 10, False)), thr


def test_gpu_subject_roi_on_a_side_stream(bare_engine):
    """The plane is produced on a side stream right before the call and the box consumed on it right after: the engine orders itself on both ends."""
    import roi_suite as RS
    import trimap_suite as TS
    base = torch.from_numpy(TS.blobs(11, 1, 300, 500) * RS.rect(300, 500, 60, 200, 100, 420)[0]).cuda()
    want = RS.brute_force((base * 0.9).cpu().numpy(), 0.3, 7, 10, True)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        plane = base * 0.9
        roi = bare_engine.subject_roi(plane, 0.3, 7, 10, True, sync=False)
        doubled = roi * 2
    st.synchronize()
    assert np.array_equal(doubled.cpu().numpy(), want * 2)


def test_gpu_subject_roi_argument_checks(bare_engine):
    import roi_suite as RS
    RS.check_subject_roi_errors(bare_engine, lambda t: t.cuda())
    RS.check_subject_roi_errors(bare_engine, lambda t: t)


def test_gpu_subject_roi_memory_is_counted_and_released(bare_engine):
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    p = torch.rand(2, 256, 256)
    bare_engine.subject_roi(p.cuda())
    mid = bare_engine.resident_bytes()
    assert mid >= bare_engine.weight_bytes() + 2 * 16                    # the raw extrema live in the arena
    bare_engine.subject_roi(p)
    assert bare_engine.resident_bytes() >= mid + 2 * 256 * 256 * 4 + 2 * 16      # host pointers: staging in and out
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()


def test_gpu_apply_matte_roi_equals_composition(loaded_engine):
    """The emulator equalities on the real kernels (tiny architecture), device pointers: every output mode with mask_refine on and off."""
    import roi_suite as RS
    RS.check_roi_call_equals_composition(loaded_engine, lambda t: t.cuda())


def test_gpu_apply_matte_roi_batch_of_two_and_host_pointers(loaded_engine):
    import roi_suite as RS
    two = ((10, 50, 20, 70), (30, 70, 50, 100))
    RS.check_roi_call_equals_composition(loaded_engine, lambda t: t.cuda(), modes=("matted_rgb", "matted_rgba"), refines=(True, ), rects=two)
    RS.check_roi_call_equals_composition(loaded_engine, lambda t: t, modes=("matted_rgb", ), refines=(True, ), rects=two)


def test_gpu_apply_matte_roi_from_mask_copy_shortcut_and_empty(loaded_engine):
    import roi_suite as RS
    for to_tensor in (lambda t: t.cuda(), lambda t: t):
        RS.check_roi_call_from_mask(loaded_engine, to_tensor)
        RS.check_roi_call_copy_shortcut(loaded_engine, to_tensor)
        RS.check_roi_call_empty(loaded_engine, to_tensor)


def test_gpu_apply_matte_roi_independence_and_errors(loaded_engine):
    import roi_suite as RS
    RS.check_roi_call_independent_of_outside(loaded_engine, lambda t: t.cuda())
    RS.check_roi_call_errors(loaded_engine, lambda t: t.cuda())
    RS.check_roi_call_errors(loaded_engine, lambda t: t)


@pytest.mark.parametrize("rects", [((20, 60, 30, 90), ), ((10, 50, 20, 70), (30, 70, 50, 100))], ids=["B1", "B2"])
def test_gpu_apply_matte_roi_profile_shows_each_launch_once(loaded_engine, rects):
    import roi_suite as RS
    image, trimap = RS.e2e_inputs(rects)
    loaded_engine.profile(True)
    loaded_engine.apply_matte_roi(image.cuda(), trimap.cuda(), 64, False, "alpha_only", True, 0.8, **RS.BOX_ARGS)
    loaded_engine.profile(False)
    res = loaded_engine.profile_results()
    assert {k: res[k]["launches"] for k in res if k.startswith("roi_")} == {k: 1 for k in RS.ROI_CALL_KERNELS}, sorted(res)
    dump = loaded_engine.profile_dump()
    assert all(dump.count(k + ",") == 1 for k in RS.ROI_CALL_KERNELS)
    assert loaded_engine.last_forward_ms() > 0.0
