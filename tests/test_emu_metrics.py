"""Matte metrics on the kernel emulator: the kernels of csrc/k_metrics.h and the labelling kernels they drive (ragged tiles and runs, tile seams, every
radius, Conn on and off) through sdm_matte_metrics with host pointers, on an engine that never loaded weights.  The real-kernel versions are
tests/test_gpu_metrics.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _emu_engine():
    from emu.build_emu import build
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Bindings, Engine
    return Engine(SDMatteConfig.tiny(), 0, True, _lib=Bindings(ctypes.CDLL(build())), precision="fp16")


@pytest.fixture(scope="module")
def emu(pkg):
    eng = _emu_engine()
    yield eng
    eng.close()


def _call(eng):
    return lambda pred, gt, tri, sigma, conn, levels: eng.matte_metrics(pred, gt, tri, grad_sigma=sigma, conn=conn, return_levels=levels)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def test_emu_metrics_case_list_and_launch_counts(emu):
    """Every case against loop_reference(fp64) under the suite's rule (n, max|e| and the level map exactly); the launch counts of the whole run are a
    function of with_conn alone."""
    import metrics_suite as MS
    MS.check_case_properties()
    emu.lib.kernel_counts(reset=True)
    MS.check(_call(emu), lambda t: t)
    assert emu.lib.kernel_counts() == MS.expected_counts(MS.case_calls())


def test_emu_metrics_launches_do_not_depend_on_size_content_or_level_output(emu):
    """2 launches without Conn, 63 with it: the same for the generic case and the one with five empty levels, with and without the level map."""
    import metrics_suite as MS
    seen = []
    for name in ("generic_2x70x133", "empty_levels_40x70", "border_s4"):
        _, pred, gt, tri, sigma, _ = MS.case(name)
        for conn, levels in ((True, True), (True, False), (False, False)):
            emu.lib.kernel_counts(reset=True)
            emu.matte_metrics(_t(pred), _t(gt), _t(tri), grad_sigma=sigma, conn=conn, return_levels=levels)
            assert emu.lib.kernel_counts() == MS.launches(conn, levels), (name, conn, levels)
            seen.append(sum(emu.lib.kernel_counts().values()))
    assert set(seen) == {2, 63}


def test_emu_metrics_exact_zeros_and_null_trimap(emu):
    """pred == gt: every sum and the maximum are exactly 0.  Trimap all 0: n and the region sums exactly 0, the frame sums not, mse 0 and not NaN.  No trimap
    is a plane of 0.5, bit for bit."""
    import metrics_suite as MS
    _, pred, gt, tri, sigma, _ = MS.case("identity_37x70")
    res = emu.matte_metrics(_t(pred), _t(gt), _t(tri), return_levels=True)
    assert float(res["raw"][0, 0]) > 100 and torch.equal(res["raw"][:, 1:], torch.zeros(1, 7, dtype=torch.float64))
    _, pred, gt, tri, sigma, _ = MS.case("empty_region_37x70")
    res = emu.matte_metrics(_t(pred), _t(gt), _t(tri))
    assert torch.equal(res["raw"][:, :6], torch.zeros(1, 6, dtype=torch.float64)) and float(res["raw"][0, 6]) > 0 and float(res["raw"][0, 7]) > 0
    assert float(res["mse"][0]) == 0.0 and float(res["sad"][0]) == 0.0 and float(res["sad_frame"][0]) > 0
    _, pred, gt, tri, sigma, _ = MS.case("dirty_2x33x70")
    a = emu.matte_metrics(_t(pred), _t(gt), None, return_levels=True)
    b = emu.matte_metrics(_t(pred), _t(gt), torch.full(pred.shape, 0.5), return_levels=True)
    assert torch.equal(a["raw"], b["raw"]) and torch.equal(a["levels"], b["levels"]) and float(a["raw"][0, 0]) == pred[0].size
    assert torch.equal(a["raw"][:, 1], a["raw"][:, 6]) and torch.equal(a["raw"][:, 2], a["raw"][:, 7])      # the region is the frame: the same tiles, the same order


@pytest.mark.parametrize("sigma", [1.4, 4.0])
def test_emu_metrics_batch_and_repeat(emu, sigma):
    """An image alone and as image 2 of a batch of 3, and the same call twice: all 8 doubles and the level map bit for bit."""
    import metrics_suite as MS
    pred3, gt3, tri3 = (_t(x) for x in MS.batch_of_three())
    whole = emu.matte_metrics(pred3, gt3, tri3, grad_sigma=sigma, return_levels=True)
    again = emu.matte_metrics(pred3, gt3, tri3, grad_sigma=sigma, return_levels=True)
    assert torch.equal(whole["raw"], again["raw"]) and torch.equal(whole["levels"], again["levels"])
    for b in range(3):
        one = emu.matte_metrics(pred3[b:b + 1].contiguous(), gt3[b:b + 1].contiguous(), tri3[b:b + 1].contiguous(), grad_sigma=sigma, return_levels=True)
        assert torch.equal(one["raw"], whole["raw"][b:b + 1]) and torch.equal(one["levels"], whole["levels"][b:b + 1]), b
    assert not torch.equal(whole["raw"][0], whole["raw"][2])


def test_emu_metrics_argument_checks_and_memory(emu):
    """Every limit on both sides: ValueError from Python, SDM_ERR_INVALID from the C ABI with nothing queued or written; never SDM_ERR_STATE without
    weights; what the call keeps is counted by resident_bytes and given back by release_memory."""
    from comfyui_sdmatte_amd.engine import _ptr
    pred, gt, tri = torch.rand(2, 20, 24), torch.rand(2, 20, 24), torch.full((2, 20, 24), 0.5)
    nan = float("nan")
    for kw in ({"grad_sigma": 0.2}, {"grad_sigma": 4.5}, {"grad_sigma": nan}, {"conn": False, "return_levels": True}):
        with pytest.raises(ValueError):
            emu.matte_metrics(pred, gt, tri, **kw)
    for args in ((pred, gt[:, :19], tri), (pred, gt, tri[:1]), (pred[0], gt[0], tri[0])):
        with pytest.raises(ValueError):
            emu.matte_metrics(*args)
    for kw in ({"grad_sigma": 0.25}, {"grad_sigma": 4.0}):
        emu.matte_metrics(pred, gt, tri, conn=False, **kw)
    stats, level = torch.full((2, 8), -7.0, dtype=torch.float64), torch.full((2, 20, 24), -7, dtype=torch.int32)

    def raw(B=2, H=20, W=24, sigma=1.4, conn=1, lev=level, kind=0):
        return emu.lib.sdm_matte_metrics(emu.h, _ptr(pred), _ptr(gt), _ptr(tri), B, H, W, sigma, conn, _ptr(stats), _ptr(lev), kind, None)
    emu.lib.kernel_counts(reset=True)
    for kw, word in (({"sigma": 0.2}, b"grad_sigma"), ({"sigma": 4.5}, b"grad_sigma"), ({"sigma": nan}, b"grad_sigma"), ({"conn": 2}, b"with_conn"),
                     ({"conn": -1}, b"with_conn"), ({"conn": 0}, b"level_bhw"), ({"kind": 7}, b"ptr_kind"), ({"H": 32769}, b"too large"),
                     ({"B": 1 << 14, "H": 1 << 7, "W": (1 << 7) + 1}, b"too large"), ({"H": 0}, b"bad image size"), ({"B": 0}, b"bad image size")):
        assert raw(**kw) == -1 and word in emu.lib.sdm_last_error(emu.h), kw
    assert emu.lib.kernel_counts() == {} and bool((stats == -7.0).all()) and bool((level == -7).all())      # nothing queued or written
    assert raw() == 0
    want = emu.matte_metrics(pred, gt, tri, return_levels=True)
    assert torch.equal(stats, want["raw"]) and torch.equal(level, want["levels"])
    assert raw(conn=0, lev=None) == 0 and torch.equal(stats[:, [0, 1, 2, 3, 5, 6, 7]], want["raw"][:, [0, 1, 2, 3, 5, 6, 7]]) and bool((stats[:, 4] == 0).all())
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    assert raw() == 0                      # host pointers: 3 planes staged in, the level map out; Q, label, root, area and the levels in the arena
    assert emu.resident_bytes() >= emu.weight_bytes() + 2 * 20 * 24 * 4 * (3 + 1 + 5)
    emu.release_memory()
    assert emu.resident_bytes() == emu.weight_bytes()
    emu.matte_metrics(pred, gt)                                             # ... and the next call allocates again
