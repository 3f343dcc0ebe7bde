"""Mask clean-up on the MI355X (csrc/k_cclabel.h through sdm_clean_mask): bit-exact against the run-based reference of tests/cleanmask_suite.py.
No model is loaded: the file stays cheap (durations in profiles/NOTES.md)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

LABEL = {"cc_tile": 1, "cc_seam": 1, "cc_flatten": 1}


@pytest.fixture(scope="module")
def bare_engine(pkg):
    """An engine that never loads weights: sdm_clean_mask needs none."""
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)
    yield eng
    eng.close()


def test_gpu_clean_mask_case_list_device_pointers(bare_engine):
    """Device tensors on torch's current stream (sync=False: result and statistics are read through that stream, as the stream contract promises)."""
    import cleanmask_suite as CS
    CS.check_clean_mask(lambda m, *p: bare_engine.clean_mask(m, *p, sync=False, return_stats=True), lambda t: t.cuda())


def test_gpu_clean_mask_case_list_host_pointers(bare_engine):
    import cleanmask_suite as CS
    CS.check_clean_mask(lambda m, *p: bare_engine.clean_mask(m, *p, return_stats=True), lambda t: t)


def test_gpu_clean_mask_on_a_side_stream(bare_engine):
    """The mask is produced on a side stream right before the call and the result consumed on it right after: the engine orders itself on both ends."""
    import cleanmask_suite as CS
    host = CS.blobs(11, 1, 300, 500)
    base = torch.from_numpy(host).cuda()
    want, wstats = CS.reference(host * np.float32(0.9), 0.5, 12, False, 12, False)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        mask = base * 0.9
        out, stats = bare_engine.clean_mask(mask, 0.5, 12, False, 12, sync=False, return_stats=True)
        doubled, stats2 = out * 2.0, stats * 2
    st.synchronize()
    assert CS.same_bits(doubled.cpu().numpy(), want * np.float32(2.0)) and np.array_equal(stats2.cpu().numpy(), wstats * 2)


def test_gpu_clean_mask_1080p_vs_reference(bare_engine):
    import cleanmask_suite as CS
    mask = CS.blobs(21, 1, 1080, 1920, n=9)
    for p in ((0.5, 64, False, 64, False), (0.5, 0, True, 1 << 28, True)):
        got, stats = bare_engine.clean_mask(torch.from_numpy(mask).cuda(), *p, return_stats=True)
        want, wstats = CS.reference(mask, *p)
        assert CS.same_bits(got.cpu().numpy(), want), (p, int((got.cpu().numpy() != want).sum()))
        assert np.array_equal(stats.cpu().numpy(), wstats), (p, stats.tolist(), wstats.tolist())
        assert wstats[0, 1] > 100 and wstats[0, 2] > 10


def test_gpu_clean_mask_launch_counts(bare_engine):
    """The launches depend on the enabled stages only: the same for a 1-pixel-wide serpentine at 257 x 515 and a batch of three small blob masks."""
    import cleanmask_suite as CS
    a = torch.from_numpy(CS._serpentine(1, 257, 515)).cuda()
    b = torch.from_numpy(CS.blobs(3, 3, 40, 33)).cuda()
    stage_a = dict(LABEL, cc_select=2, cc_apply=1)
    both = dict(cc_tile=2, cc_seam=2, cc_flatten=2, cc_select=2, cc_apply=1, cc_fill=1)
    for p, stats, want in (((0.5, 0, False, 0, False), False, {"cc_apply": 1}), ((0.5, 0, False, 0, True), True, dict(LABEL, cc_apply=1)),
                           ((0.5, 2, False, 0, False), False, stage_a), ((0.5, 0, True, 0, False), True, stage_a),
                           ((0.5, 0, False, 1, False), False, dict(LABEL, cc_apply=1, cc_fill=1)), ((0.5, 64, True, 64, False), True, both)):
        seen = []
        for m in (a, b):
            bare_engine.lib.kernel_counts(reset=True)
            bare_engine.clean_mask(m, *p, return_stats=stats)
            seen.append(bare_engine.lib.kernel_counts())
        assert seen[0] == seen[1] == want, (p, stats, seen)
    bare_engine.profile(True)
    bare_engine.clean_mask(a, 0.5, 64, False, 64)
    bare_engine.profile(False)
    res = bare_engine.profile_results()
    assert {k: v["launches"] for k, v in res.items() if k.startswith("cc_")} == both, sorted(res)


def test_gpu_clean_mask_then_make_trimap_on_one_stream(bare_engine):
    """The chain the call exists for, without a host synchronisation in between: clean_mask, then make_trimap, on torch's current stream."""
    import cleanmask_suite as CS
    import trimap_suite as TS
    blob, raw = CS.purpose_masks()
    cleaned = bare_engine.clean_mask(torch.from_numpy(raw).cuda(), 0.5, 64, False, 64, sync=False)
    tri = bare_engine.make_trimap(cleaned, 0.5, 10, 10, sync=False)
    tri_raw = bare_engine.make_trimap(torch.from_numpy(raw).cuda(), 0.5, 10, 10, sync=False)
    want = TS.brute_force(blob, 0.5, 10, 10)
    assert np.array_equal(cleaned.cpu().numpy(), blob) and np.array_equal(tri.cpu().numpy(), want)
    assert int((tri_raw.cpu().numpy() != want).sum()) > 1000


def test_gpu_clean_mask_batch_memory_and_restatement(bare_engine):
    """B = 3 equals three single calls and the CPU restatement; the label planes are counted and released."""
    import cleanmask_suite as CS
    from comfyui_sdmatte_amd.sdmatte_nodes import clean_mask
    bare_engine.release_memory()
    base = bare_engine.resident_bytes()
    mask = torch.from_numpy(np.concatenate([CS.blobs(8, 1, 333, 517), CS._rings(1, 333, 517), CS._batch_pair(1, 333, 517)]))
    got, st = bare_engine.clean_mask(mask.cuda(), 0.5, 6, True, 30, return_stats=True)
    assert bare_engine.resident_bytes() >= base + 3 * 333 * 517 * 12
    want, wst = clean_mask(mask, 0.5, 6, True, 30, return_stats=True)
    assert CS.same_bits(got.cpu().numpy(), want.numpy()) and torch.equal(st.cpu(), wst)
    for i in range(3):
        one, st1 = bare_engine.clean_mask(mask[i:i + 1].cuda(), 0.5, 6, True, 30, return_stats=True)
        assert torch.equal(got[i:i + 1], one) and torch.equal(st[i:i + 1], st1), i
    bare_engine.release_memory()
    assert bare_engine.resident_bytes() == base
    with pytest.raises(ValueError):
        bare_engine.clean_mask(mask.cuda(), 1.0)
