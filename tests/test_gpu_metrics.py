"""Matte metrics on the MI355X (csrc/k_metrics.h and the labelling kernels of csrc/k_cclabel.h through sdm_matte_metrics) against the loop reference of
tests/metrics_suite.py under its tolerance rule.  No weights, no oracle forward: the file stays cheap (ratios and durations in profiles/NOTES.md)."""
import functools
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
    """An engine that never loads weights: sdm_matte_metrics needs none."""
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)
    yield eng
    eng.close()


def _call(eng, **kw):
    return lambda pred, gt, tri, sigma, conn, levels: eng.matte_metrics(pred, gt, tri, grad_sigma=sigma, conn=conn, return_levels=levels, **kw)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _same(a, b):
    return torch.equal(a["raw"].cpu(), b["raw"].cpu()) and torch.equal(a["levels"].cpu(), b["levels"].cpu())


def test_gpu_metrics_case_list_device_pointers(bare_engine):
    """Device tensors on torch's current stream (sync=False: the results are read through that stream, as the stream contract promises); the launch
    counts of the whole run are a function of with_conn alone."""
    import metrics_suite as MS
    MS.check_case_properties()
    bare_engine.lib.kernel_counts(reset=True)
    MS.check(_call(bare_engine, sync=False), lambda t: t.cuda())
    assert bare_engine.lib.kernel_counts() == MS.expected_counts(MS.case_calls())


def test_gpu_metrics_case_list_host_pointers(bare_engine):
    import metrics_suite as MS
    MS.check(_call(bare_engine), lambda t: t)


def test_gpu_metrics_on_a_side_stream(bare_engine):
    """The inputs are produced on a side stream right before the call and the results consumed on it right after: the engine orders itself on both ends."""
    import metrics_suite as MS
    pred, gt, tri = (_t(x) for x in MS.batch_of_three())
    want = bare_engine.matte_metrics(pred * 0.5, gt * 0.5, tri, return_levels=True)
    base = [t.cuda() for t in (pred, gt, tri)]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        ins = [base[0] * 0.5, base[1] * 0.5, base[2] * 1.0]
        got = bare_engine.matte_metrics(*ins, return_levels=True, sync=False)
        raw2, lev2 = got["raw"] * 1.0, got["levels"] + 0
    st.synchronize()
    assert torch.equal(raw2.cpu(), want["raw"]) and torch.equal(lev2.cpu(), want["levels"])
    assert float(want["raw"][:, 1].min()) > 0 and 1 <= int(want["levels"].max()) <= 5


@pytest.mark.parametrize("sigma", [0.25, 1.4, 4.0])
def test_gpu_metrics_batch_pointer_kind_and_repeat(bare_engine, sigma):
    """An image alone and as image 2 of a batch of 3, host and device pointers, the same call twice: all 8 doubles and the level map bit for bit."""
    import metrics_suite as MS
    host = [_t(x) for x in MS.batch_of_three()]
    dev = [t.cuda() for t in host]
    got = bare_engine.matte_metrics(*dev, grad_sigma=sigma, return_levels=True)
    assert _same(got, bare_engine.matte_metrics(*dev, grad_sigma=sigma, return_levels=True))
    h = bare_engine.matte_metrics(*host, grad_sigma=sigma, return_levels=True)
    assert h["raw"].device.type == "cpu" and h["levels"].device.type == "cpu" and _same(h, got)
    for b in range(3):
        for src in (host, dev):
            one = bare_engine.matte_metrics(*(t[b:b + 1].contiguous() for t in src), grad_sigma=sigma, return_levels=True)
            assert torch.equal(one["raw"].cpu(), got["raw"][b:b + 1].cpu()) and torch.equal(one["levels"].cpu(), got["levels"][b:b + 1].cpu()), b
    nc = bare_engine.matte_metrics(*dev, grad_sigma=sigma, conn=False)
    keep = [0, 1, 2, 3, 5, 6, 7]
    assert torch.equal(nc["raw"][:, keep], got["raw"][:, keep]) and bool((nc["raw"][:, 4] == 0).all())


def test_gpu_metrics_exact_zeros_and_null_trimap(bare_engine):
    """pred == gt: every sum and the maximum exactly 0.  Trimap all 0: n and the region sums exactly 0, the frame sums not, mse 0 and not NaN.  No trimap is
    a plane of 0.5, bit for bit."""
    import metrics_suite as MS
    _, pred, gt, tri, _, _ = MS.case("identity_37x70")
    res = bare_engine.matte_metrics(_t(pred).cuda(), _t(gt).cuda(), _t(tri).cuda(), return_levels=True)
    assert float(res["raw"][0, 0]) > 100 and torch.equal(res["raw"][:, 1:].cpu(), torch.zeros(1, 7, dtype=torch.float64))
    _, pred, gt, tri, _, _ = MS.case("empty_region_37x70")
    res = bare_engine.matte_metrics(_t(pred).cuda(), _t(gt).cuda(), _t(tri).cuda())
    assert torch.equal(res["raw"][:, :6].cpu(), torch.zeros(1, 6, dtype=torch.float64)) and float(res["raw"][0, 6]) > 0 and float(res["raw"][0, 7]) > 0
    assert float(res["mse"][0]) == 0.0 and float(res["sad_frame"][0]) > 0
    _, pred, gt, tri, _, _ = MS.case("dirty_2x33x70")
    a = bare_engine.matte_metrics(_t(pred).cuda(), _t(gt).cuda(), None, return_levels=True)
    b = bare_engine.matte_metrics(_t(pred).cuda(), _t(gt).cuda(), torch.full(pred.shape, 0.5).cuda(), return_levels=True)
    assert _same(a, b) and float(a["raw"][0, 0]) == pred[0].size


@functools.lru_cache(maxsize=None)
def _scene_200():
    """(pred, gt, trimap, raw64, levels, d32) of 2 x 200 x 200 at sigma 4.  The reference here is the torch restatement on fp64 tensors, not the loop
    reference (which would take minutes at this size); `metrics_suite.check_references_agree` ties the two together on every case of the list.  d32 comes
    from the restatement on fp32 tensors and from `variant32`, as in the suite."""
    import metrics_suite as MS
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    pred, gt, tri = MS._generic(31, 2, 200, 200)
    tp, tg, tt = _t(pred), _t(gt), _t(tri)
    ref = N.matte_metrics(tp.double(), tg.double(), tt.double(), 4.0, True, return_levels=True)
    r64, lev = ref["raw"].numpy(), ref["levels"].numpy()
    d32 = np.maximum(np.abs(N.matte_metrics(tp, tg, tt, 4.0, True)["raw"].numpy() - r64), np.abs(MS.variant32(pred, gt, tri, 4.0, True, lev) - r64))
    return tp, tg, tt, r64, lev, d32


@pytest.mark.parametrize("conn", [True, False])
def test_gpu_metrics_200x200_accuracy(bare_engine, conn):
    """2 x 200 x 200 (7 x 4 tiles of mm_pixel, 16 tiles of the labelling, 10 runs) at sigma 4: n, max|e| and the levels exactly, the sums to the suite's
    rule (reference: see _scene_200)."""
    import metrics_suite as MS
    tp, tg, tt, r64, lev, d32 = _scene_200()
    got = bare_engine.matte_metrics(tp.cuda(), tg.cuda(), tt.cuda(), grad_sigma=4.0, conn=conn, return_levels=conn)
    raw = got["raw"].cpu().numpy()
    assert np.array_equal(raw[:, 0], r64[:, 0]) and np.array_equal(raw[:, 5], r64[:, 5].astype(np.float32).astype(np.float64))
    if conn:
        assert np.array_equal(got["levels"].cpu().numpy(), lev) and len(np.unique(lev)) >= 8
    for b in range(2):
        for s in MS.SUM_SLOTS:
            want = r64[b, s] if (conn or s != 4) else 0.0
            d, tol = abs(raw[b, s] - want), MS.tolerance(d32[b, s], want)
            line = f"[metrics] 2x200x200 conn={conn} image {b} {MS.SLOT_NAMES[s]}: d32 = {d32[b, s]:.3e} tol = {tol:.3e} d = {d:.3e}"
            print(line)
            assert d <= tol, line


@pytest.mark.parametrize("conn", [True, False])
def test_gpu_metrics_profile_shows_the_documented_launches(bare_engine, conn):
    import metrics_suite as MS
    tp, tg, tt = (_t(x).cuda() for x in MS._generic(31, 2, 200, 200))
    bare_engine.profile(True)
    bare_engine.matte_metrics(tp, tg, tt, grad_sigma=4.0, conn=conn, return_levels=conn)
    bare_engine.profile(False)
    res = bare_engine.profile_results()
    assert {k: v["launches"] for k, v in res.items()} == MS.launches(conn), res
    assert bare_engine.last_forward_ms() > 0.0


def test_gpu_metrics_argument_errors_queue_and_write_nothing(bare_engine):
    """SDM_ERR_INVALID from the C ABI with device pointers: prefilled outputs untouched, no launch counted; the good call then writes both."""
    import metrics_suite as MS
    from comfyui_sdmatte_amd.engine import _ptr
    dp, dg, dt = (_t(x).cuda() for x in MS._generic(31, 2, 200, 200))
    stats, level = torch.full((2, 8), -7.0, dtype=torch.float64).cuda(), torch.full((2, 200, 200), -7, dtype=torch.int32).cuda()

    def raw_call(B=2, H=200, W=200, sigma=1.4, conn=1, lev=level, kind=1):
        return bare_engine.lib.sdm_matte_metrics(bare_engine.h, _ptr(dp), _ptr(dg), _ptr(dt), B, H, W, sigma, conn, _ptr(stats), _ptr(lev), kind, None)
    torch.cuda.synchronize()
    bare_engine.lib.kernel_counts(reset=True)
    for kw in ({"sigma": 0.2}, {"sigma": 4.5}, {"sigma": float("nan")}, {"conn": 2}, {"conn": 0}, {"kind": 7}, {"B": 1 << 14, "H": 1 << 7, "W": (1 << 7) + 1}):
        assert raw_call(**kw) == -1, kw
    bare_engine.synchronize()
    assert bare_engine.lib.kernel_counts() == {} and bool((stats == -7.0).all()) and bool((level == -7).all())
    assert raw_call() == 0
    bare_engine.synchronize()
    assert bool((stats[:, 0] > 0).all()) and bool((level >= 0).all())
