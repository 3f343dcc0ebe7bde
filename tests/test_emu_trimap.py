"""Trimap from a mask on the kernel emulator: the two kernels of csrc/k_trimap.h (index math, halos, ragged edges, the wave-uniform
shortcuts) against the brute force, and sdm_apply_matte_mask against sdm_make_trimap + sdm_apply_matte_node on the tiny architecture.
The real-kernel versions are tests/test_gpu_trimap.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _emu_engine(cfg=None):
    from emu.build_emu import build
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Bindings, Engine
    return Engine(cfg or SDMatteConfig.tiny(), 0, True, _lib=Bindings(ctypes.CDLL(build())), precision="fp16")


def test_emu_make_trimap_equals_brute_force(pkg):
    """Every case of the list at 97x131 and 5x300 (no tile multiples), B = 2, host pointers, on an engine that never loaded weights."""
    import trimap_suite as TS
    eng = _emu_engine()
    eng.lib.kernel_counts(reset=True)
    TS.check_make_trimap(lambda m, thr, e, d: eng.make_trimap(m, thr, e, d), lambda t: t)
    n = len(TS.small_cases())
    counts = eng.lib.kernel_counts()
    assert counts == {"trimap_cols": n, "trimap_rows": n}, counts
    eng.close()


def test_emu_make_trimap_equals_cpu_restatement_and_reuses_out(pkg):
    """GPU kernels (emulated), CPU restatement and brute force agree bit for bit; `out=` is filled in place; one-pixel and one-row images are legal."""
    import trimap_suite as TS
    from comfyui_sdmatte_amd.sdmatte_nodes import trimap_from_mask
    eng = _emu_engine()
    mask = torch.from_numpy(TS.blobs(3, 3, 70, 67))                     # B = 3, a different mask per image
    out = torch.full((3, 70, 67), -1.0)
    got = eng.make_trimap(mask, 0.45, 6, 11, out=out)
    assert got is out and torch.equal(out, trimap_from_mask(mask, 0.45, 6, 11))
    assert np.array_equal(out.numpy(), TS.brute_force(mask.numpy(), 0.45, 6, 11))
    for shape in ((1, 1, 1), (1, 1, 300), (2, 130, 1), (1, 257, 3)):
        m = torch.rand(*shape, generator=torch.Generator().manual_seed(shape[1]))
        assert torch.equal(eng.make_trimap(m, 0.5, 2, 40), torch.from_numpy(TS.brute_force(m.numpy(), 0.5, 2, 40))), shape
    eng.close()


def test_emu_make_trimap_argument_checks_and_memory(pkg):
    """Out-of-range radii raise (Python check and SDM_ERR_INVALID of the C ABI); no SDM_ERR_STATE without weights; what the call keeps is counted
    by resident_bytes and given back by release_memory."""
    eng = _emu_engine()
    m = torch.rand(1, 20, 30)
    for bad in ((-1, 3), (3, 256), (1000, 1), (2.5, 3)):
        with pytest.raises(ValueError):
            eng.make_trimap(m, 0.5, *bad)
    with pytest.raises(ValueError):
        eng.make_trimap(torch.rand(20, 30))
    with pytest.raises(ValueError):
        eng.make_trimap(m, out=torch.empty(1, 20, 29))
    out = torch.empty(1, 20, 30)
    from comfyui_sdmatte_amd.engine import _ptr
    for e, d in ((256, 0), (0, -1)):
        rc = eng.lib.sdm_make_trimap(eng.h, _ptr(m), 1, 20, 30, 0.5, e, d, _ptr(out), 0, None)
        assert rc == -1 and b"outside 0 .. 255" in eng.lib.sdm_last_error(eng.h), rc
    assert eng.lib.sdm_make_trimap(eng.h, _ptr(m), 1, 0, 30, 0.5, 1, 1, _ptr(out), 0, None) == -1
    assert eng.resident_bytes() == eng.weight_bytes()                    # nothing kept so far
    eng.make_trimap(m, 0.5, 3, 3)
    assert eng.resident_bytes() > eng.weight_bytes()                     # distance plane (arena) + host staging
    eng.release_memory()
    assert eng.resident_bytes() == eng.weight_bytes()
    eng.make_trimap(m, 0.5, 3, 3)                                        # ... and the next call allocates again
    eng.close()


def test_emu_apply_matte_mask_equals_make_trimap_then_node(pkg):
    """Tiny architecture, image 50x70 at inference size 64: sdm_apply_matte_mask == sdm_make_trimap + sdm_apply_matte_node bit for bit in alpha,
    matted and trimap, for every output mode with mask_refine on and off; the trimap kernels run once per call; no SDM_ERR_ARENA (the generated trimap
    and the distance plane are arena allocations of both passes); a mask of another size passes or raises by apply_matte_node's rule."""
    import trimap_suite as TS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.weights import synthetic_state_dict
    cfg = SDMatteConfig.tiny()
    eng = _emu_engine(cfg)
    eng.load_state_dict(synthetic_state_dict(cfg, 0))
    TS.check_mask_call_equals_two_calls(eng, lambda t: t)
    image, mask = TS.e2e_inputs()
    with pytest.raises(ValueError):
        eng.apply_matte_mask(image, mask, 64, False, "alpha_only", False, 0.8, 0.5, 300, 1)
    with pytest.raises(ValueError):
        eng.apply_matte_mask(image, mask, 64, False, "nope", False, 0.8)
    with pytest.raises(ValueError):
        eng.apply_matte_mask(image[..., :2], mask, 64, False, "alpha_only", False, 0.8)
    eng.close()


def test_emu_fan_out_apply_matte_mask(pkg):
    """MultiGpuEngine.apply_matte_mask splits the batch like apply_matte_node (same bits as one engine fed the same shards); make_trimap runs on the
    first engine."""
    import trimap_suite as TS
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.parallel import MultiGpuEngine
    from comfyui_sdmatte_amd.weights import synthetic_state_dict
    cfg = SDMatteConfig.tiny()
    w = synthetic_state_dict(cfg, 0)
    one = _emu_engine(cfg)
    one.load_state_dict(w)
    fan = MultiGpuEngine(cfg, [0, 1], _engine_factory=lambda d: _emu_engine(cfg))
    fan.load_state_dict(w)
    image, mask = TS.e2e_inputs(B=2, H=64, W=64)
    fa, fm, ft = fan.apply_matte_mask(image, mask, 64, False, "matted_rgba", True, 0.8, 0.4, 3, 5)
    for i in range(2):
        a, m, t = one.apply_matte_mask(image[i:i + 1], mask[i:i + 1], 64, False, "matted_rgba", True, 0.8, 0.4, 3, 5)
        assert torch.equal(fa[i:i + 1], a) and torch.equal(fm[i:i + 1], m) and torch.equal(ft[i:i + 1], t)
    assert torch.equal(fan.make_trimap(mask, 0.4, 3, 5), ft)
    one.close(); fan.close()
