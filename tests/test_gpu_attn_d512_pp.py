"""-m gpu: the ping-pong form of the d = 512 attention kernel (option attn512_pp, k_attn.h attn_d512_pp_kernel; VAE mid-block).  The block's two wave halves
run the same MFMAs on the same operands in the same order as attn_d512_kernel, one phase apart: every case is checked against fp64 attention at the kernel's
existing tolerance AND bit for bit (torch.equal) against attn_d512_kernel, for fp16 and fp32 results - one key tile, two, an odd count, a ragged last tile, a
late jump of the running maximum; a ragged query block and two whole ones."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ops_suite as S      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOL = 5e-3                # tests/test_gpu_ops.py::test_attention_d512
CASES = [(Lq, Lk, False) for Lq in (130, 256) for Lk in (32, 64, 96, 301)] + [(Lq, 64, True) for Lq in (130, 256)]


@pytest.fixture(scope="module")
def eng(pkg):
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.config import SDMatteConfig
    e = Engine(SDMatteConfig.tiny(), 0, True)
    yield e
    e.close()


@pytest.mark.parametrize("Lq,Lk,spike", CASES)
def test_ping_pong_against_fp64_and_the_lock_step_kernel(eng, engine_option, Lq, Lk, spike):
    seed = 1000 * Lq + 10 * Lk + int(spike)
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(2, n, 512, generator=g).half() for n in (Lq, Lk, Lk))
    if spike:
        k[:, Lk - 3] = (q[:, 0].float() * 4.0).half()      # a large jump of the running maximum in the last tile (the rescale branch)
    s = torch.matmul(q.double(), k.double().transpose(-1, -2)) * 512 ** -0.5
    ref = torch.matmul(s.softmax(-1), v.double()).float()
    q, k, v = q.to(DEV), k.to(DEV), v.to(DEV)
    out = {}
    for opt in (1, 0):
        engine_option(eng, "attn512_pp", opt)
        eng.lib.kernel_counts(reset=True)
        err = S.check_attention(eng, DEV, 2, 1, Lq, Lk, 512, use_bias=False, spike=spike, atol=ATOL, seed=seed)      # fp16 result, the suite's own operands
        out[opt] = (eng.op_attention(q, k, v, 1).cpu(), eng.op_attention_f32(q, k, v, 1).cpu())
        assert eng.lib.kernel_counts().get("attn_d512_pp", 0) == 3 * opt, (opt, eng.lib.kernel_counts())
        e16, e32 = ((o.float() - ref).abs().max().item() for o in out[opt])
        print(f"\n[attn512_pp = {opt}] Lq={Lq} Lk={Lk} spike={spike}: max |out - fp64| suite {err:.3e}, fp16 {e16:.3e}, fp32 {e32:.3e}")
        assert e16 < ATOL and e32 < ATOL, (opt, e16, e32)
    assert torch.equal(out[1][0], out[0][0]), (out[1][0].float() - out[0][0].float()).abs().max().item()
    assert torch.equal(out[1][1], out[0][1]), (out[1][1] - out[0][1]).abs().max().item()
