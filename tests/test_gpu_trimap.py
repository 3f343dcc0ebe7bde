"""Trimap from a mask on the MI355X (csrc/k_trimap.h through sdm_make_trimap / sdm_apply_matte_mask): bit-exact against the references of
tests/trimap_suite.py.  Tiny architecture only, no oracle forward: the file stays cheap (durations in profiles/NOTES.md)."""
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
    """An engine that never loads weights: sdm_make_trimap needs none."""
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)
    yield eng
    eng.close()


def test_gpu_make_trimap_case_list_device_pointers(bare_engine):
    """Device tensors on torch's current stream (sync=False: the result is read through that stream, as the stream contract promises)."""
    import trimap_suite as TS
    TS.check_make_trimap(lambda m, thr, e, d: bare_engine.make_trimap(m, thr, e, d, sync=False), lambda t: t.cuda())


def test_gpu_make_trimap_case_list_host_pointers(bare_engine):
    import trimap_suite as TS
    TS.check_make_trimap(lambda m, thr, e, d: bare_engine.make_trimap(m, thr, e, d), lambda t: t)


def test_gpu_make_trimap_on_a_side_stream(bare_engine):
    """The mask is produced on a side stream right before the call and the trimap consumed on it right after: the engine orders itself on both ends."""
    import trimap_suite as TS
    base = torch.from_numpy(TS.blobs(11, 1, 300, 500)).cuda()
    want = TS.brute_force((base * 0.9).cpu().numpy(), 0.5, 5, 9)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        mask = base * 0.9
        tri = bare_engine.make_trimap(mask, 0.5, 5, 9, sync=False)
        doubled = tri * 2.0
    st.synchronize()
    assert np.array_equal(doubled.cpu().numpy(), want * 2.0)


def test_gpu_make_trimap_1080p_vs_brute_force(bare_engine):
    import trimap_suite as TS
    mask = TS.blobs(21, 1, 1080, 1920, n=9)
    got = bare_engine.make_trimap(torch.from_numpy(mask).cuda(), 0.5, 10, 20).cpu().numpy()
    want = TS.brute_force(mask, 0.5, 10, 20)
    assert np.array_equal(got, want), int((got != want).sum())
    assert {0.0, 0.5, 1.0} == set(np.unique(got).tolist())


@pytest.mark.parametrize("H,W,r", [(2048, 1536, 64), (700, 900, 255)])
def test_gpu_make_trimap_large_radius_vs_separable(bare_engine, H, W, r):
    import trimap_suite as TS
    mask = TS.blobs(H + r, 1, H, W, n=9)
    got = bare_engine.make_trimap(torch.from_numpy(mask).cuda(), 0.5, r, r).cpu().numpy()
    want = TS.separable(mask, 0.5, r, r)
    assert np.array_equal(got, want), int((got != want).sum())


def test_gpu_make_trimap_batch_of_three_and_cpu_restatement(bare_engine):
    """B = 3 with a different mask per image: each equals its own single-image trimap, the brute force and the CPU restatement."""
    import trimap_suite as TS
    from comfyui_sdmatte_amd.sdmatte_nodes import trimap_from_mask
    mask = torch.from_numpy(TS.blobs(31, 3, 333, 517))
    assert not torch.equal(mask[0], mask[1]) and not torch.equal(mask[1], mask[2])
    got = bare_engine.make_trimap(mask.cuda(), 0.45, 7, 12).cpu()
    assert np.array_equal(got.numpy(), TS.brute_force(mask.numpy(), 0.45, 7, 12))
    assert torch.equal(got, trimap_from_mask(mask, 0.45, 7, 12))
    for b in range(3):
        assert torch.equal(got[b:b + 1], bare_engine.make_trimap(mask[b:b + 1].cuda(), 0.45, 7, 12).cpu())


def test_gpu_make_trimap_memory_is_counted_and_released(bare_engine):
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    m = torch.rand(1, 256, 256)
    bare_engine.make_trimap(m.cuda(), 0.5, 4, 4)
    mid = bare_engine.resident_bytes()
    assert mid >= bare_engine.weight_bytes() + 256 * 256 * 2              # the distance plane lives in the arena
    bare_engine.make_trimap(m, 0.5, 4, 4)
    assert bare_engine.resident_bytes() >= mid + 2 * 256 * 256 * 4       # host pointers: staging in and out
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == bare_engine.weight_bytes()
    with pytest.raises(ValueError):
        bare_engine.make_trimap(m.cuda(), 0.5, 256, 0)


def test_gpu_apply_matte_mask_equals_make_trimap_then_node(pkg):
    """The emulator end-to-end equalities on the real kernels (tiny architecture), device pointers and host pointers; the two launches show in the
    per-launch profile."""
    import trimap_suite as TS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.weights import synthetic_state_dict
    cfg = SDMatteConfig.tiny()
    eng = Engine(cfg, 0)
    eng.load_state_dict(synthetic_state_dict(cfg, 0))
    TS.check_mask_call_equals_two_calls(eng, lambda t: t.cuda(), B=2)
    TS.check_mask_call_equals_two_calls(eng, lambda t: t, modes=("matted_rgb",), refines=(True,))
    image, mask = TS.e2e_inputs()
    eng.profile(True)
    eng.apply_matte_mask(image.cuda(), mask.cuda(), 64, False, "alpha_only", True, 0.8, 0.4, 3, 5)
    eng.profile(False)
    res = eng.profile_results()
    assert res["trimap_cols"]["launches"] == 1 and res["trimap_rows"]["launches"] == 1, sorted(res)
    assert "trimap_cols," in eng.profile_dump() and "trimap_rows," in eng.profile_dump()
    eng.close()
