"""Tiles along the unknown band and the node call that blends them on the MI355X (csrc/k_tiles.h through sdm_band_tiles / sdm_apply_matte_tiles): against
the references of tests/tiles_suite.py, with device and host pointers.  Tiny architecture only, no oracle forward: the file stays cheap."""
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
    """An engine that never loads weights: sdm_band_tiles needs none."""
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


def test_gpu_band_tiles_case_list_device_pointers(bare_engine):
    import tiles_suite as TS
    TS.check_band_tiles(bare_engine, lambda t: t.cuda())


def test_gpu_band_tiles_case_list_host_pointers(bare_engine):
    import tiles_suite as TS
    TS.check_band_tiles(bare_engine, lambda t: t)


def test_gpu_band_tiles_unaligned_device_pointer(bare_engine):
    """96 x 128 on a device tensor sliced so that its pointer is not 16-byte aligned: the scalar path, the same tiles."""
    import roi_suite as RS
    import tiles_suite as TS
    cases = [c for c in TS.band_cases() if c[0].startswith("ring_96x128")]
    assert len(cases) == 5
    TS.check_band_tiles(bare_engine, lambda t: RS.misaligned(t.cuda()), cases)


def test_gpu_band_tiles_many_blocks_per_image(bare_engine):
    """1080 x 1920, B = 2: 127 blocks per image meet in the flag words."""
    import tiles_suite as TS
    cases = [c for c in TS.band_cases(big=True) if c[0] == "many_blocks_1080x1920"]
    assert len(cases) == 1
    TS.check_band_tiles(bare_engine, lambda t: t.cuda(), cases)


def test_gpu_band_tiles_on_a_side_stream(bare_engine):
    """The trimap is produced on a side stream right before the call and the list consumed on it right after: the engine orders itself on both ends."""
    import tiles_suite as TS
    base = torch.from_numpy(TS.ring(300, 517)).cuda()
    want, wcnt = TS.brute_force((base * 0.9).cpu().numpy(), 0.3, 0.6, 256, 32, 16)
    assert 0 < int(wcnt[0]) <= 16
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        plane = base * 0.9
        tiles, cnt = bare_engine.band_tiles(plane, 0.3, 0.6, 256, 32, 16, sync=False, return_count=True)
        doubled, cnt2 = tiles * 2, cnt + 1
    st.synchronize()
    assert np.array_equal(doubled.cpu().numpy(), want * 2) and np.array_equal(cnt2.cpu().numpy(), wcnt + 1)


def test_gpu_band_tiles_argument_checks(bare_engine):
    import tiles_suite as TS
    TS.check_band_tiles_errors(bare_engine, lambda t: t.cuda())
    TS.check_band_tiles_errors(bare_engine, lambda t: t)


def test_gpu_band_tiles_memory_is_counted_and_released(bare_engine):
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    p = torch.rand(2, 256, 256)
    bare_engine.band_tiles(p.cuda())
    mid = bare_engine.resident_bytes()
    assert mid >= bare_engine.weight_bytes() + 2 * 8 * 4                               # the flag words live in the arena
    bare_engine.band_tiles(p)
    assert bare_engine.resident_bytes() >= mid + 2 * 256 * 256 * 4 + 2 * 16 * 20       # host pointers: staging in and out
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()


def test_gpu_band_tiles_profile_shows_the_launches(bare_engine):
    import tiles_suite as TS
    plane = torch.from_numpy(TS.ring(300, 517)).cuda()
    bare_engine.profile(True)
    bare_engine.band_tiles(plane, tile=64, overlap=16)
    bare_engine.profile(False)
    res = bare_engine.profile_results()
    assert {k: res[k]["launches"] for k in res} == {k: 1 for k in TS.BAND_KERNELS}, sorted(res)
    assert bare_engine.last_forward_ms() > 0.0


def test_gpu_apply_matte_tiles_equals_node_call(loaded_engine):
    """One tile = the frame: bit-identical to apply_matte_node for every output mode with mask_refine on and off, device and host pointers."""
    import tiles_suite as TS
    TS.check_equals_node_call(loaded_engine, lambda t: t.cuda())
    TS.check_equals_node_call(loaded_engine, lambda t: t)


def test_gpu_apply_matte_tiles_disjoint_tiles_are_exact(loaded_engine):
    import tiles_suite as TS
    TS.check_disjoint_tiles(loaded_engine, lambda t: t.cuda())
    TS.check_disjoint_tiles(loaded_engine, lambda t: t, (("matted_rgb", True), ))


def test_gpu_apply_matte_tiles_overlapping_tiles(loaded_engine):
    import tiles_suite as TS
    TS.check_overlapping_tiles(loaded_engine, lambda t: t.cuda())


def test_gpu_apply_matte_tiles_mixed_order_and_base(loaded_engine):
    import tiles_suite as TS
    TS.check_mixed_order_and_base(loaded_engine, lambda t: t.cuda())
    TS.check_mixed_order_and_base(loaded_engine, lambda t: t, modes=TS.MODES_OV[1:], modes_base=TS.MODES_OV[:1])


def test_gpu_apply_matte_tiles_structure(loaded_engine):
    """Equal slot values, N = 0, void entries among valid ones."""
    import tiles_suite as TS
    for to_tensor in (lambda t: t.cuda(), lambda t: t):
        TS.check_constant_slots(loaded_engine, to_tensor)
        TS.check_no_tiles(loaded_engine, to_tensor)
        TS.check_void_entries(loaded_engine, to_tensor)


def test_gpu_apply_matte_tiles_errors(loaded_engine):
    import tiles_suite as TS
    TS.check_call_errors(loaded_engine, lambda t: t.cuda())
    TS.check_call_errors(loaded_engine, lambda t: t)


def test_gpu_apply_matte_tiles_on_a_side_stream(loaded_engine):
    """Inputs produced on a side stream right before the call, outputs consumed on it right after, sync=False."""
    import boxes_suite as BS
    import tiles_suite as TS
    image, trimap = BS.frames(1, seed=27)
    tiles = TS.tiles_tensor([[0, 4, 8, 48, 56], [0, 30, 50, 48, 56]])
    want_a, want_m = TS.call(loaded_engine, lambda t: t.cuda(), image * 0.5, trimap, tiles, "matted_rgba", True, 6)
    img2, tri, lst = (image * 0.25).cuda(), trimap.cuda(), (tiles // 2).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        a, m = loaded_engine.apply_matte_tiles(img2 * 2, tri, lst * 2 + (tiles % 2).cuda(), 64, False, "matted_rgba", True, 0.8, 6, sync=False)
        a2, m2 = a * 2, m * 2
    st.synchronize()
    assert torch.equal(a2, want_a * 2) and torch.equal(m2, want_m * 2)


def test_gpu_apply_matte_tiles_memory_is_counted_and_released(loaded_engine):
    import boxes_suite as BS
    import tiles_suite as TS
    image, trimap = BS.frames(1, seed=28)
    tiles = TS.tiles_tensor([[0, 5, 8, 40, 48], [0, 50, 70, 40, 48]])
    loaded_engine.release_memory()
    assert loaded_engine.resident_bytes() == loaded_engine.weight_bytes()
    TS.call(loaded_engine, lambda t: t.cuda(), image, trimap, tiles)
    mid = loaded_engine.resident_bytes()
    assert mid > loaded_engine.weight_bytes() + 2 * 2 * 64 * 64 * 16 * 2               # at least the model's input planes of batch N = 2
    TS.call(loaded_engine, lambda t: t, image, trimap, tiles, base=trimap)
    assert loaded_engine.resident_bytes() >= mid + 96 * 128 * 20 + 2 * 20 + 96 * 128 * 16      # host pointers: image, trimap, base and list in, alpha and matted out
    loaded_engine.release_memory()
    assert loaded_engine.resident_bytes() == loaded_engine.weight_bytes()


@pytest.mark.parametrize("entries", [[], [[0, 20, 30, 40, 60]], [[0, 5, 8, 40, 48], [0, 30, 40, 40, 48], [0, 20, 40, 50, 50]]], ids=["N0", "N1", "N3"])
def test_gpu_apply_matte_tiles_profile_shows_each_launch_once(loaded_engine, entries):
    import boxes_suite as BS
    import tiles_suite as TS
    image, trimap = BS.frames(1, seed=29)
    want = TS.CALL_KERNELS if entries else ("tiles_blend", )
    loaded_engine.profile(True)
    TS.call(loaded_engine, lambda t: t.cuda(), image, trimap, TS.tiles_tensor(entries), "alpha_only", True, 4)
    loaded_engine.profile(False)
    res = loaded_engine.profile_results()
    assert {k: res[k]["launches"] for k in res if k.startswith(("boxes_", "tiles_"))} == {k: 1 for k in want}, sorted(res)
    dump = loaded_engine.profile_dump()
    assert all(dump.count(k + ",") == 1 for k in want)
    assert loaded_engine.last_forward_ms() > 0.0
