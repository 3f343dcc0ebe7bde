"""The ping-pong form of the d = 512 attention kernel (option attn512_pp, k_attn.h attn_d512_pp_kernel) on the kernel emulator: an odd tile count with a ragged
last key tile and a ragged query block, against fp64 attention and bit for bit against attn_d512_kernel.  (The emulator executes an LDS-DMA where it is issued:
a DMA issued while a wave still has to read the buffer it overwrites would show here; one that lands too late would not.)"""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ops_suite as S      # noqa: E402


def _q_k_v(B, Lq, Lk, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, n, 512, generator=g).half() for n in (Lq, Lk, Lk))


def test_ping_pong_equals_the_lock_step_kernel(pkg, engine_option):
    from emu.build_emu import build
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Bindings, Engine
    eng = Engine(SDMatteConfig.tiny(), 0, True, _lib=Bindings(ctypes.CDLL(build())))
    try:
        q, k, v = _q_k_v(1, 130, 96, 71)
        out = {}
        for opt in (1, 0):
            engine_option(eng, "attn512_pp", opt)
            eng.lib.kernel_counts(reset=True)
            S.check_attention(eng, "cpu", 1, 1, 130, 96, 512, use_bias=False, atol=5e-3, seed=72)
            out[opt] = (eng.op_attention(q, k, v, 1), eng.op_attention_f32(q, k, v, 1))
            assert eng.lib.kernel_counts().get("attn_d512_pp", 0) == 3 * opt, (opt, eng.lib.kernel_counts())
        assert torch.equal(out[1][0], out[0][0]) and torch.equal(out[1][1], out[0][1])
        assert bool(torch.isfinite(out[1][1]).all()) and (out[1][1] - out[1][0].float()).abs().max().item() < 2e-3      # fp16 rounding of values < 4
    finally:
        eng.close()
