"""The narrow form of the d = 64 attention cores on the shared cross-attention operand (option cross_narrow, k_attn.h NARROW) on the kernel emulator:
the ones rows of the operand, and the whole cross-attention of a block - q_shared -> core -> out_shared - bit for bit against the full d = 64 program, on the
ping-pong kernel and the 4-wave pipeline at one and nine key tiles."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_emu_folds import _engine, _setup      # noqa: E402  (the tiny architecture with non-zero folded biases)

BLOCK = "unet.mid_block.attentions.0"           # C = 128, two heads


@pytest.fixture(scope="module")
def eng(pkg):
    cfg, w = _setup()
    e = _engine(cfg, w, "fp16x3")
    yield e
    e.close()


def test_ones_rows_of_the_patch_planes(eng):
    g = torch.Generator().manual_seed(61)
    for shape in ((2, 8, 8), (1, 5, 7)):                                   # 64 keys: no padding column; 35 keys: 29 of them
        B, H, W = shape
        L, ldvt = H * W, (H * W + 63) // 64 * 64
        uin = torch.randn(B, H, W, 16, generator=g)
        k0, p0, v0 = eng.op_cross_patch_planes(uin)
        k1, p1, v1 = eng.op_cross_patch_planes(uin, ones_rows=True)
        assert torch.equal(k0, k1) and torch.equal(p0, p1), shape          # K and its pair plane stay as they are
        assert v1.shape == (B, 64, ldvt) and torch.equal(v1[:, :36], v0[:, :36]), shape
        want = torch.zeros(B, 28, ldvt, dtype=torch.float16)
        want[:, [59 - 36, 63 - 36], :L] = 1.0
        assert torch.equal(v1[:, 36:], want), shape
        assert bool((v0[:, 36:] == 0).all()), shape


@pytest.mark.parametrize("form", ["pp", "pipe4"])
@pytest.mark.parametrize("grid", [(8, 8), (24, 24)])
def test_narrow_equals_full(eng, engine_option, grid, form):
    if form == "pp":
        engine_option(eng, "attn_pp_min_blocks", 0)
    else:
        engine_option(eng, "attn_nw", 4)
    g = torch.Generator().manual_seed(62 + grid[0])
    x = torch.randn(2, 8, 4, 128, generator=g)
    uin = torch.randn(2, grid[0], grid[1], 16, generator=g)
    out, counts = {}, {}
    for opt in (1, 0):
        engine_option(eng, "cross_narrow", opt)
        eng.lib.kernel_counts(reset=True)
        out[opt] = eng.debug_cross_attention(BLOCK, x, uin)
        counts[opt] = eng.lib.kernel_counts(reset=True)
    kernel = "attn_d64_pp" if form == "pp" else "attn_d64_pipe<4>"
    assert counts[1].get("attn_d64_narrow", 0) == 1 and counts[0].get("attn_d64_narrow", 0) == 0, (counts[1], counts[0])
    assert counts[1].get(kernel, 0) == 1 and counts[0].get(kernel, 0) == 1, (counts[1], counts[0])
    assert bool(torch.isfinite(out[1]).all()) and out[1].abs().max().item() > 0
    assert torch.equal(out[1], out[0]), (grid, form, (out[1] - out[0]).abs().max().item())
