"""Mask clean-up on the kernel emulator: the kernels of csrc/k_cclabel.h (tile labelling in LDS, seam unions, flatten, selection, apply / fill)
through Engine.clean_mask against the run-based reference of tests/cleanmask_suite.py, bit for bit.  The real-kernel versions are
tests/test_gpu_cleanmask.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

HOST, DEVICE, INVALID = 0, 1, -1      # SDM_PTR_HOST, SDM_PTR_DEVICE, SDM_ERR_INVALID (include/sdmatte.h)
LABEL = {"cc_tile": 1, "cc_seam": 1, "cc_flatten": 1}


@pytest.fixture(scope="module")
def eng(pkg):
    """An engine on the emulated library that never loads weights: sdm_clean_mask needs none."""
    from emu.build_emu import build
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Bindings, Engine
    e = Engine(SDMatteConfig.tiny(), 0, True, _lib=Bindings(ctypes.CDLL(build())), precision="fp16")
    yield e
    e.close()


def _raw(eng, mask, p, kind, stats=True):
    """sdm_clean_mask itself, with the pointer kind of the caller's choice -> (rc, out, stats)."""
    from comfyui_sdmatte_amd.engine import _ptr
    mask = mask.float().contiguous()
    B, H, W = mask.shape
    out = torch.empty(B, H, W)
    st = torch.empty(B, 4, dtype=torch.int32) if stats else None
    rc = eng.lib.sdm_clean_mask(eng.h, _ptr(mask), B, H, W, p[0], p[1], int(p[2]), p[3], int(p[4]), _ptr(out), _ptr(st), kind, None)
    eng.synchronize()
    return rc, out, st


def test_emu_clean_mask_case_list_device_pointers(eng):
    """The whole list (every pattern at every shape, B = 1 and 3) through Engine.clean_mask; on the emulator its pointers count as device pointers."""
    import cleanmask_suite as CS
    assert eng._kind(torch.zeros(1)) == DEVICE
    CS.check_clean_mask(lambda m, *p: eng.clean_mask(m, *p, return_stats=True), lambda t: t)


def test_emu_clean_mask_case_list_host_pointers(eng):
    """The same through the I/O staging (SDM_PTR_HOST): the statistics are the second staged output."""
    import cleanmask_suite as CS

    def call(m, *p):
        rc, out, st = _raw(eng, m, p, HOST)
        assert rc == 0, eng.lib.sdm_last_error(eng.h)
        return out, st
    CS.check_clean_mask(call, lambda t: t)


def test_emu_clean_mask_without_stats_and_out_reuse(eng):
    import cleanmask_suite as CS
    mask = torch.from_numpy(CS.blobs(5, 2, 70, 131))
    want, _ = CS.reference(mask.numpy(), 0.4, 9, False, 7, False)
    out = torch.full((2, 70, 131), -1.0)
    got = eng.clean_mask(mask, 0.4, 9, False, 7, out=out)
    assert got is out and CS.same_bits(out.numpy(), want)
    rc, got, _ = _raw(eng, mask, (0.4, 9, False, 7, False), HOST, stats=False)
    assert rc == 0 and CS.same_bits(got.numpy(), want)
    from comfyui_sdmatte_amd.sdmatte_nodes import clean_mask
    assert CS.same_bits(clean_mask(mask, 0.4, 9, False, 7).numpy(), want)


def test_emu_clean_mask_launches_depend_on_the_stages_only(eng):
    """Two masks of different size, batch and content launch the same kernels under the same stages; the stage sets launch what the header says."""
    import cleanmask_suite as CS
    a = torch.from_numpy(CS._serpentine(1, 257, 515))
    b = torch.from_numpy(CS.blobs(3, 3, 40, 33))
    stage_a = dict(LABEL, cc_select=2, cc_apply=1)
    stage_b = dict(LABEL, cc_fill=1)
    both = {k: stage_a.get(k, 0) + stage_b.get(k, 0) for k in set(stage_a) | set(stage_b)}
    for p, stats, want in (((0.5, 0, False, 0, False), False, {"cc_apply": 1}), ((0.5, 1, False, 0, True), False, {"cc_apply": 1}),
                           ((0.5, 0, False, 0, False), True, dict(LABEL, cc_apply=1)),
                           ((0.5, 2, False, 0, False), False, stage_a), ((0.5, 0, True, 0, False), False, stage_a), ((0.5, 64, True, 0, True), True, stage_a),
                           ((0.5, 0, False, 1, False), False, dict(stage_b, cc_apply=1)), ((0.5, 1, False, 99, False), True, dict(both, cc_select=0)),
                           ((0.5, 64, False, 64, False), False, both), ((0.5, 64, True, 64, True), True, both)):
        seen = []
        for m in (a, b):
            eng.lib.kernel_counts(reset=True)
            eng.clean_mask(m, *p, return_stats=stats)
            seen.append(eng.lib.kernel_counts())
        assert seen[0] == seen[1] == {k: v for k, v in want.items() if v}, (p, stats, seen)


def test_emu_clean_mask_batch_equals_single_calls(eng):
    import cleanmask_suite as CS
    mask = torch.from_numpy(np.concatenate([CS.blobs(8, 1, 90, 75), CS._rings(1, 90, 75), CS._batch_pair(1, 90, 75)]))
    for p in ((0.5, 6, False, 5, False), (0.5, 0, True, 30, True)):
        got, st = eng.clean_mask(mask, *p, return_stats=True)
        for i in range(3):
            one, st1 = eng.clean_mask(mask[i:i + 1], *p, return_stats=True)
            assert CS.same_bits(got[i:i + 1].numpy(), one.numpy()) and torch.equal(st[i:i + 1], st1), (p, i)


def test_emu_clean_mask_argument_errors_write_nothing(eng):
    """Every argument outside its limits: SDM_ERR_INVALID, no launch, and output and statistics buffers keep their poison - for both pointer kinds."""
    from comfyui_sdmatte_amd.engine import _ptr
    m = torch.rand(2, 20, 30)
    good = dict(B=2, H=20, W=30, thr=0.5, min_area=4, keep=0, hole=4, binz=0)
    bad = [dict(thr=1.0), dict(thr=-0.01), dict(thr=float("nan")), dict(thr=float("inf")), dict(thr=1.5), dict(min_area=-1), dict(min_area=(1 << 28) + 1),
           dict(hole=-1), dict(hole=(1 << 28) + 1), dict(keep=2), dict(keep=-1), dict(binz=2), dict(binz=-1), dict(B=0), dict(H=0), dict(W=0), dict(W=-3),
           dict(H=32769, W=1, B=1), dict(H=1, W=32769, B=1), dict(B=5, H=16384, W=16384)]
    for kind in (HOST, DEVICE):
        for change in bad:
            a = dict(good, **change)
            out = torch.full((2, 20, 30), 7.5)
            st = torch.full((2, 4), -9, dtype=torch.int32)
            eng.lib.kernel_counts(reset=True)
            rc = eng.lib.sdm_clean_mask(eng.h, _ptr(m), a["B"], a["H"], a["W"], a["thr"], a["min_area"], a["keep"], a["hole"], a["binz"], _ptr(out), _ptr(st), kind,
                                        None)
            assert rc == INVALID and eng.lib.sdm_last_error(eng.h).startswith(b"clean mask"), (change, rc)
            assert eng.lib.kernel_counts() == {} and bool((out == 7.5).all()) and bool((st == -9).all()), change
    assert eng.lib.sdm_clean_mask(eng.h, _ptr(m), 2, 20, 30, 0.5, 4, 0, 4, 0, _ptr(torch.empty(2, 20, 30)), None, 7, None) == INVALID      # pointer kind
    assert eng.lib.sdm_clean_mask(eng.h, None, 2, 20, 30, 0.5, 4, 0, 4, 0, _ptr(torch.empty(2, 20, 30)), None, HOST, None) == INVALID
    assert eng.lib.sdm_clean_mask(eng.h, _ptr(m), 2, 20, 30, 0.5, 4, 0, 4, 0, None, None, HOST, None) == INVALID
    for kw in (dict(threshold=1.0), dict(threshold=-1.0), dict(min_area=-1), dict(max_hole_area=1 << 29), dict(min_area=1.5)):
        with pytest.raises(ValueError):
            eng.clean_mask(m, **kw)
    with pytest.raises(ValueError):
        eng.clean_mask(m[0])
    with pytest.raises(ValueError):
        eng.clean_mask(m, out=torch.empty(2, 20, 29))
    # the limits themselves are legal
    out, st = eng.clean_mask(m, float(np.nextafter(np.float32(1), np.float32(0))), 1 << 28, True, 1 << 28, True, return_stats=True)
    assert bool((out == 0).all())


def test_emu_clean_mask_memory_is_counted_and_released(eng):
    """No SDM_ERR_STATE on a context without weights; the three label planes (12 bytes per pixel, arena) and the host staging are counted by
    resident_bytes and given back by release_memory."""
    eng.release_memory()
    assert eng.weight_bytes() == 0 or eng.resident_bytes() == eng.weight_bytes()
    base = eng.resident_bytes()
    m = torch.rand(1, 100, 128)
    eng.clean_mask(m, 0.5, 0, False, 0)                                  # both stages off, no statistics: no plane at all
    assert eng.resident_bytes() == base
    eng.clean_mask(m, 0.5, 4, False, 4)
    mid = eng.resident_bytes()
    assert mid >= base + 100 * 128 * 12
    rc, _, _ = _raw(eng, m, (0.5, 4, False, 4, False), HOST)
    assert rc == 0 and eng.resident_bytes() >= mid + 2 * 100 * 128 * 4 + 16      # staging: mask in, mask and statistics out
    eng.release_memory()
    assert eng.resident_bytes() == base
    eng.clean_mask(m, 0.5, 4, False, 4)                                  # ... and the next call allocates again
    eng.release_memory()


def test_emu_clean_mask_serves_its_purpose(eng):
    """A blob with three 5-pixel islands and two 4-pixel pin-holes: the trimap (10 / 10) of the cleaned mask is the trimap of the blob alone; the
    trimap of the raw mask differs from it in more than 1000 pixels."""
    import cleanmask_suite as CS
    blob, raw = CS.purpose_masks()
    assert int((raw != blob).sum()) == 3 * 5 + 2 * 4
    cleaned, st = eng.clean_mask(torch.from_numpy(raw), 0.5, 64, False, 64, return_stats=True)
    assert st.tolist() == [[4, 3, 2, 23]] and np.array_equal(cleaned.numpy(), blob)
    want = eng.make_trimap(torch.from_numpy(blob), 0.5, 10, 10)
    assert torch.equal(eng.make_trimap(cleaned, 0.5, 10, 10), want)
    assert int((eng.make_trimap(torch.from_numpy(raw), 0.5, 10, 10) != want).sum()) > 1000


def test_emu_fan_out_clean_mask(eng, pkg):
    """MultiGpuEngine.clean_mask runs on the first engine, like make_trimap."""
    import cleanmask_suite as CS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Bindings, Engine
    from comfyui_sdmatte_amd.parallel import MultiGpuEngine
    cfg = SDMatteConfig.tiny()
    fan = MultiGpuEngine(cfg, [0, 1], _engine_factory=lambda d: Engine(cfg, 0, True, _lib=eng.lib, precision="fp16"))
    mask = torch.from_numpy(CS.blobs(2, 2, 50, 60))
    got, st = fan.clean_mask(mask, 0.5, 6, True, 5, return_stats=True)
    want, wst = CS.reference(mask.numpy(), 0.5, 6, True, 5, False)
    assert CS.same_bits(got.numpy(), want) and np.array_equal(st.numpy(), wst)
    assert torch.equal(fan.clean_mask(mask, 0.5, 6, True, 5), got)
    fan.close()
