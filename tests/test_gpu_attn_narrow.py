"""-m gpu: the narrow form of the d = 64 attention cores on the shared cross-attention operand (option cross_narrow, k_attn.h NARROW).
The operand has 36 live columns: the narrow form drops the Q.K^T step over K columns 48..63 (products with a zero operand) and reads the softmax denominator
from a row of ones in V^T instead of from MFMAs of its own - the same sums in the same order, so everything behind out_shared is BIT-IDENTICAL between
cross_narrow = 1 and 0.  Checked with torch.equal on the ping-pong kernel, the 4-wave pipeline and the key split, at one, four and nine key tiles and 8192
keys; a key count that is no multiple of 64 keeps the full program; and end to end against the oracle."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
TOL = 1e-3          # BASELINE.json north_star: alpha within 1e-3 max abs of the reference CPU path
BLOCK = "unet.mid_block.attentions.0"      # tiny architecture: C = 128, two heads
N_TRANSFORMER_BLOCKS = 16
KEY_GRIDS = {64: (8, 8), 256: (16, 16), 576: (24, 24), 8192: (64, 128), 100: (10, 10)}      # key count -> latent grid of the U-Net input


@pytest.fixture(scope="module")
def eng(pkg):
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.weights import synthetic_state_dict
    cfg = SDMatteConfig.tiny()
    e = Engine(cfg, 0, True)
    e.weights = synthetic_state_dict(cfg, 3)
    e.load_state_dict(e.weights)
    yield e
    e.close()


def _uin(B, h, w, seed):
    return torch.randn(B, h, w, 16, generator=torch.Generator().manual_seed(seed)).cuda()


def _both(eng, engine_option, run):
    """run() under cross_narrow = 1 and 0 -> ({option: result}, {option: launch counts})"""
    out, counts = {}, {}
    for opt in (1, 0):
        engine_option(eng, "cross_narrow", opt)
        eng.lib.kernel_counts(reset=True)
        out[opt] = run()
        counts[opt] = eng.lib.kernel_counts(reset=True)
    return out, counts


def _two_heads(eng, engine_option, Lk, seed):
    """The whole cross-attention of a two-head block (q_shared -> core -> out_shared), B = 2, 256 queries: the out_shared result of both forms."""
    h, w = KEY_GRIDS[Lk]
    x = torch.randn(2, 16, 16, 128, generator=torch.Generator().manual_seed(seed)).cuda()
    u = _uin(2, h, w, seed + 100)
    out, counts = _both(eng, engine_option, lambda: eng.debug_cross_attention(BLOCK, x, u))
    assert bool(torch.isfinite(out[1]).all()) and out[1].abs().max().item() > 0
    assert torch.equal(out[1], out[0]), (Lk, (out[1] - out[0]).abs().max().item())
    assert counts[0].get("attn_d64_narrow", 0) == 0, counts[0]
    return counts[1]


def _five_heads(eng, engine_option, Lk, seed):
    """The core alone on the engine's operand at five heads (no block of the tiny architecture has them), B = 2, 256 queries: the 36 columns per head that
    out_shared reads are equal; columns 59 and 63 are the denominator over itself in the narrow form and zero in the full one."""
    h, w = KEY_GRIDS[Lk]
    q = torch.randn(2, 256, 5, 64, generator=torch.Generator().manual_seed(seed)) * 2.0
    q[..., 36:] = 0
    q = q.reshape(2, 256, 320).cuda()
    u = _uin(2, h, w, seed + 100)
    out, counts = _both(eng, engine_option, lambda: eng.op_cross_core(q, u, 5).view(2, 256, 5, 64))
    assert bool(torch.isfinite(out[1]).all()) and out[1][..., :36].abs().max().item() > 0
    assert torch.equal(out[1][..., :36], out[0][..., :36]), (Lk, (out[1] - out[0])[..., :36].abs().max().item())
    assert counts[0].get("attn_d64_narrow", 0) == 0, counts[0]
    if counts[1].get("attn_d64_narrow", 0):
        dead = [c for c in range(36, 64) if c not in (59, 63)]
        assert bool((out[1][..., dead] == 0).all()) and bool((out[0][..., 36:] == 0).all())
        assert (out[1][..., [59, 63]] - 1.0).abs().max().item() <= 2.0 ** -22      # l * (1 / l): one rounding of the reciprocal, one of the product
    return counts[1]


@pytest.mark.parametrize("Lk", [64, 256, 576])
def test_narrow_equals_full_on_the_ping_pong_kernel(eng, engine_option, Lk):
    engine_option(eng, "attn_pp_min_blocks", 0)
    for c in (_two_heads(eng, engine_option, Lk, 41), _five_heads(eng, engine_option, Lk, 42)):
        assert c.get("attn_d64_narrow", 0) == 1 and c.get("attn_d64_pp", 0) == 1 and c.get("attn_combine", 0) == 0, c


@pytest.mark.parametrize("Lk", [64, 256, 576])
def test_narrow_equals_full_on_the_four_wave_pipeline(eng, engine_option, Lk):
    engine_option(eng, "attn_nw", 4)
    for c in (_two_heads(eng, engine_option, Lk, 43), _five_heads(eng, engine_option, Lk, 44)):
        assert c.get("attn_d64_narrow", 0) == 1 and c.get("attn_d64_pipe<4>", 0) == 1 and c.get("attn_combine", 0) == 0, c


@pytest.mark.parametrize("form", ["pp", "pipe4"])
@pytest.mark.parametrize("nsplit", [2, 4])
def test_narrow_equals_full_with_a_key_split(eng, engine_option, nsplit, form):
    if form == "pp":
        engine_option(eng, "attn_pp_min_blocks", 0)
    else:
        engine_option(eng, "attn_nw", 4)
    engine_option(eng, "attn_ksplit", nsplit)
    kernel = "attn_d64_pp" if form == "pp" else "attn_d64_pipe<4>"
    for c in (_two_heads(eng, engine_option, 8192, 45 + nsplit), _five_heads(eng, engine_option, 8192, 46 + nsplit)):
        assert c.get("attn_d64_narrow", 0) == 1 and c.get(kernel, 0) == 1 and c.get(f"attn_combine/n={nsplit}", 0) == 1, c


def test_a_ragged_key_count_keeps_the_full_program(eng, engine_option):
    engine_option(eng, "attn_pp_min_blocks", 0)
    for c in (_two_heads(eng, engine_option, 100, 51), _five_heads(eng, engine_option, 100, 52)):
        assert c.get("attn_d64_narrow", 0) == 0 and c.get("attn_d64_pipe<4>", 0) == 1, c


def test_end_to_end_against_the_oracle(eng, engine_option):
    from comfyui_sdmatte_amd.synth import synthetic_inputs
    from oracle import sdmatte_oracle as O
    img, tri = synthetic_inputs(2, 256, 256, seed=9)
    data = {"image": (img.permute(0, 3, 1, 2).contiguous() - 0.5) / 0.5, "trimap": tri.unsqueeze(1) * 2 - 1,
            "is_trans": torch.tensor([0, 1]), "trimap_coords": torch.tensor([[0.0, 0.0, 1.0, 1.0]] * 2)}
    ref = O.sdmatte_forward(eng.weights, eng.cfg.as_dict(), data)
    out, counts = _both(eng, engine_option,
                        lambda: eng.forward(data["image"].cuda(), data["trimap"].cuda(), is_trans=data["is_trans"].numpy()).cpu())
    d = (out[1] - ref).abs().max().item()
    print(f"\n[cross_narrow = 1, tiny S=256 B=2] max |alpha - oracle| = {d:.3e}; narrow launches {counts[1].get('attn_d64_narrow', 0)}")
    assert d <= TOL, d
    assert counts[1].get("attn_d64_narrow", 0) == N_TRANSFORMER_BLOCKS and counts[0].get("attn_d64_narrow", 0) == 0, (counts[1], counts[0])
    assert torch.equal(out[1], out[0]), (out[1] - out[0]).abs().max().item()
