"""A box per subject and the node call over a list of boxes on the MI355X (csrc/k_boxes.h through sdm_subject_boxes / sdm_apply_matte_boxes): exact against
the references of tests/boxes_suite.py.  Tiny architecture only, no oracle forward: the file stays cheap."""
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
    """An engine that never loads weights: sdm_subject_boxes needs none."""
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


def test_gpu_subject_boxes_case_list_device_pointers(bare_engine):
    import boxes_suite as BS
    BS.check_subject_boxes(bare_engine, lambda t: t.cuda())


def test_gpu_subject_boxes_case_list_host_pointers(bare_engine):
    import boxes_suite as BS
    BS.check_subject_boxes(bare_engine, lambda t: t)


def test_gpu_subject_boxes_unaligned_device_pointer(bare_engine):
    """96 x 128 on a device tensor sliced so that its pointer is not 16-byte aligned: the same boxes."""
    import boxes_suite as BS
    import roi_suite as RS
    cases = [c for c in BS.box_cases() if c[0].startswith("vector_path_96x128")]
    assert len(cases) == 2
    BS.check_subject_boxes(bare_engine, lambda t: RS.misaligned(t.cuda()), cases)


def test_gpu_subject_boxes_many_blocks_per_image(bare_engine):
    """1080 x 1920, B = 2: 127 blocks per image meet in the atomics of the rank launches and of both reductions."""
    import boxes_suite as BS
    cases = [c for c in BS.box_cases(big=True) if c[0] == "many_blocks_1080x1920"]
    assert len(cases) == 1
    BS.check_subject_boxes(bare_engine, lambda t: t.cuda(), cases)


def test_gpu_subject_boxes_launches_depend_on_max_boxes_only(bare_engine):
    import boxes_suite as BS
    for K in (1, 2, 5, 8):
        seen = []
        for plane in (torch.zeros(1, 40, 50), torch.rand(2, 300, 517), torch.ones(1, 3, 200)):
            bare_engine.lib.kernel_counts(reset=True)
            bare_engine.subject_boxes(plane.cuda(), 0.5, 2, K)
            seen.append(bare_engine.lib.kernel_counts())
        assert seen[0] == seen[1] == seen[2] == BS.launches(K) and sum(seen[0].values()) == 8 + 2 * (K - 1)


def test_gpu_subject_boxes_on_a_side_stream(bare_engine):
    """The plane is produced on a side stream right before the call and the list consumed on it right after: the engine orders itself on both ends."""
    import boxes_suite as BS
    base = torch.from_numpy(BS.paint(300, 517, ((20, 120, 30, 200), (150, 280, 300, 500), (200, 230, 40, 90)))).cuda()
    want, wcnt = BS.brute_force((base * 0.9).cpu().numpy(), 0.3, 64, 4, 7, 10, True)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        plane = base * 0.9
        boxes, cnt = bare_engine.subject_boxes(plane, 0.3, 64, 4, 7, 10, True, sync=False, return_count=True)
        doubled, cnt2 = boxes * 2, cnt + 1
    st.synchronize()
    assert np.array_equal(doubled.cpu().numpy(), want * 2) and np.array_equal(cnt2.cpu().numpy(), wcnt + 1)


def test_gpu_subject_boxes_argument_checks(bare_engine):
    import boxes_suite as BS
    BS.check_subject_boxes_errors(bare_engine, lambda t: t.cuda())
    BS.check_subject_boxes_errors(bare_engine, lambda t: t)


def test_gpu_subject_boxes_memory_is_counted_and_released(bare_engine):
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    p = torch.rand(2, 256, 256)
    bare_engine.subject_boxes(p.cuda())
    mid = bare_engine.resident_bytes()
    assert mid >= bare_engine.weight_bytes() + 3 * 2 * 256 * 256 * 4                  # the three label planes live in the arena
    bare_engine.subject_boxes(p)
    assert bare_engine.resident_bytes() >= mid + 2 * 256 * 256 * 4 + 2 * 4 * 20        # host pointers: staging in and out
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()


def test_gpu_apply_matte_boxes_equals_roi_call(loaded_engine):
    """Equality 1, device and host pointers."""
    import boxes_suite as BS
    BS.check_equals_roi_call(loaded_engine, lambda t: t.cuda())
    BS.check_equals_roi_call(loaded_engine, lambda t: t)


def test_gpu_apply_matte_boxes_every_mode_disjoint_boxes(loaded_engine):
    """Equality 2 with two disjoint boxes in one image: every output mode with mask_refine on and off."""
    import boxes_suite as BS
    modes = tuple((m, r) for m in ("alpha_only", "matted_rgba", "matted_rgb") for r in (False, True))
    BS.check_equals_composition(loaded_engine, lambda t: t.cuda(), [[0, 5, 8, 40, 48], [0, 50, 70, 40, 48]], modes=modes)


def test_gpu_apply_matte_boxes_overlap_mixed_order_and_copy_branch(loaded_engine):
    """Two overlapping boxes (the maximum is exercised); B = 2 with three entries in mixed image order, host pointers too; a box of exactly S x S."""
    import boxes_suite as BS
    BS.check_equals_composition(loaded_engine, lambda t: t.cuda(), [[0, 10, 20, 48, 56], [0, 30, 50, 48, 56]], overlap=(30, 58, 50, 76))
    mixed = [[1, 20, 60, 44, 44], [0, 8, 8, 44, 44], [1, 40, 10, 44, 44]]
    BS.check_equals_composition(loaded_engine, lambda t: t.cuda(), mixed, B=2, modes=(("matted_rgba", True), ))
    BS.check_equals_composition(loaded_engine, lambda t: t, mixed, B=2, modes=(("matted_rgb", True), ))
    BS.check_equals_composition(loaded_engine, lambda t: t.cuda(), [[0, 16, 32, 64, 64]], modes=(("matted_rgba", True), ))


def test_gpu_apply_matte_boxes_void_entries(loaded_engine):
    import boxes_suite as BS
    BS.check_void_entries(loaded_engine, lambda t: t.cuda())
    BS.check_void_entries(loaded_engine, lambda t: t)


def test_gpu_apply_matte_boxes_errors(loaded_engine):
    import boxes_suite as BS
    BS.check_call_errors(loaded_engine, lambda t: t.cuda())
    BS.check_call_errors(loaded_engine, lambda t: t)


def test_gpu_apply_matte_boxes_on_a_side_stream(loaded_engine):
    """Inputs produced on a side stream right before the call, outputs consumed on it right after, sync=False."""
    import boxes_suite as BS
    image, trimap = BS.frames(1, seed=27)
    boxes = BS.boxes_tensor([[0, 5, 8, 40, 48], [0, 50, 70, 40, 48]])
    want_a, want_m = BS.call(loaded_engine, lambda t: t.cuda(), image * 0.5, trimap, boxes, "matted_rgba", True)
    img2, tri, lst = (image * 0.25).cuda(), trimap.cuda(), (boxes // 2).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        a, m = loaded_engine.apply_matte_boxes(img2 * 2, tri, lst * 2 + (boxes % 2).cuda(), 64, False, "matted_rgba", True, 0.8, sync=False)
        a2, m2 = a * 2, m * 2
    st.synchronize()
    assert torch.equal(a2, want_a * 2) and torch.equal(m2, want_m * 2)


def test_gpu_apply_matte_boxes_memory_is_counted_and_released(loaded_engine):
    import boxes_suite as BS
    image, trimap = BS.frames(1, seed=28)
    boxes = BS.boxes_tensor([[0, 5, 8, 40, 48], [0, 50, 70, 40, 48]])
    loaded_engine.release_memory()
    assert loaded_engine.resident_bytes() == loaded_engine.weight_bytes()
    BS.call(loaded_engine, lambda t: t.cuda(), image, trimap, boxes)
    mid = loaded_engine.resident_bytes()
    assert mid > loaded_engine.weight_bytes() + 2 * 2 * 64 * 64 * 16 * 2               # at least the model's input planes of batch N = 2
    BS.call(loaded_engine, lambda t: t, image, trimap, boxes)
    assert loaded_engine.resident_bytes() >= mid + 96 * 128 * 16 + 2 * 20 + 96 * 128 * 16      # host pointers: image, trimap and list in, alpha and matted out
    loaded_engine.release_memory()
    assert loaded_engine.resident_bytes() == loaded_engine.weight_bytes()


@pytest.mark.parametrize("entries", [[[0, 20, 30, 40, 60]], [[0, 5, 8, 40, 48], [0, 50, 70, 30, 50], [0, 20, 40, 50, 50]]], ids=["N1", "N3"])
def test_gpu_apply_matte_boxes_profile_shows_each_launch_once(loaded_engine, entries):
    import boxes_suite as BS
    image, trimap = BS.frames(1, seed=29)
    loaded_engine.profile(True)
    BS.call(loaded_engine, lambda t: t.cuda(), image, trimap, BS.boxes_tensor(entries), "alpha_only", True)
    loaded_engine.profile(False)
    res = loaded_engine.profile_results()
    assert {k: res[k]["launches"] for k in res if k.startswith("boxes_")} == {k: 1 for k in BS.CALL_KERNELS}, sorted(res)
    dump = loaded_engine.profile_dump()
    assert all(dump.count(k + ",") == 1 for k in BS.CALL_KERNELS)
    assert loaded_engine.last_forward_ms() > 0.0


def test_gpu_subject_boxes_profile_shows_the_launches(bare_engine):
    import boxes_suite as BS
    plane = torch.from_numpy(BS.paint(97, 131, BS.THREE)).cuda()
    bare_engine.profile(True)
    bare_engine.subject_boxes(plane, 0.0, 64, 4)
    bare_engine.profile(False)
    res = bare_engine.profile_results()
    assert {k: res[k]["launches"] for k in res} == BS.launches(4), sorted(res)
    assert bare_engine.last_forward_ms() > 0.0
