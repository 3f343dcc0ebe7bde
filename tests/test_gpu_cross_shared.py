"""-m gpu: cross-attention on ONE key / value operand per forward (option cross_shared).  Op level: the attention core on a shared
operand (head stride 0 for K and V^T) against the same values replicated per head through the existing path with transpose_v - bit for bit, on the
ping-pong kernel, the 4-wave pipeline and the key split.  End to end: the tiny architecture against the oracle with the launch census, and a rectangle."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
TOL = 1e-3          # BASELINE.json north_star: alpha within 1e-3 max abs of the reference CPU path
N_TRANSFORMER_BLOCKS = 16


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


def _shared_vs_replicated(eng, B, heads, Lq, Lk, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Lq, heads * 64, generator=g).cuda()
    ks = torch.randn(B, Lk, 64, generator=g)
    vs = torch.randn(B, Lk, 64, generator=g)
    ks[:, :, 36:] = 0                      # the engine's operand: 36 live columns
    vs[:, :, 36:] = 0
    ks, vs = ks.cuda(), vs.cuda()
    eng.lib.kernel_counts(reset=True)
    got = eng.op_attention_shared(q, ks, vs, heads)
    c_shared = eng.lib.kernel_counts(reset=True)
    want = eng.op_attention_split(q, ks.repeat(1, 1, heads), vs.repeat(1, 1, heads), heads)
    c_rep = eng.lib.kernel_counts(reset=True)
    assert c_shared.get("transpose_v", 0) == 0 and c_rep.get("transpose_v", 0) == 1, (c_shared, c_rep)
    assert bool(torch.isfinite(got).all()) and got.abs().max().item() > 0
    assert torch.equal(got, want), (got - want).abs().max().item()
    return c_shared, c_rep


def test_shared_equals_replicated_on_the_ping_pong_kernel(eng, engine_option):
    engine_option(eng, "attn_pp_min_blocks", 0)
    for c in _shared_vs_replicated(eng, 2, 5, 256, 512, 31):
        assert c.get("attn_d64_pp", 0) == 1 and c.get("attn_pp<0,0,0>", 0) == 1, c


def test_shared_equals_replicated_on_the_four_wave_pipeline(eng, engine_option):
    engine_option(eng, "attn_nw", 4)
    for c in _shared_vs_replicated(eng, 2, 5, 256, 512, 32):
        assert c.get("attn_d64_pipe<4>", 0) == 1, c


@pytest.mark.parametrize("nsplit", [2, 4])
def test_shared_equals_replicated_with_a_key_split(eng, engine_option, nsplit):
    engine_option(eng, "attn_ksplit", nsplit)
    for c in _shared_vs_replicated(eng, 1, 2, 256, 8192, 33 + nsplit):
        assert c.get(f"attn_combine/n={nsplit}", 0) == 1 and c.get("attn_combine", 0) == 1, c


def _forward(eng, data):
    return eng.forward(data["image"].cuda(), data["trimap"].cuda(), is_trans=data["is_trans"].numpy()).cpu()


def _data(B, H, W, seed):
    from comfyui_sdmatte_amd.synth import synthetic_inputs
    img, tri = synthetic_inputs(B, H, W, seed=seed)
    return {"image": (img.permute(0, 3, 1, 2).contiguous() - 0.5) / 0.5, "trimap": tri.unsqueeze(1) * 2 - 1,
            "is_trans": torch.tensor([0, 1][:B]), "trimap_coords": torch.tensor([[0.0, 0.0, 1.0, 1.0]] * B)}


def test_end_to_end_against_the_oracle_with_launch_census(eng, engine_option):
    from oracle import sdmatte_oracle as O
    data = _data(2, 256, 256, 9)
    ref = O.sdmatte_forward(eng.weights, eng.cfg.as_dict(), data)      # one oracle evaluation for both option values
    out, counts = {}, {}
    for opt in (1, 0):
        engine_option(eng, "cross_shared", opt)
        eng.lib.kernel_counts(reset=True)
        out[opt] = _forward(eng, data)
        counts[opt] = eng.lib.kernel_counts()
        d = (out[opt] - ref).abs().max().item()
        print(f"\n[cross_shared = {opt}, tiny S=256 B=2] max |alpha - oracle| = {d:.3e}")
        assert d <= TOL, (opt, d)
    print(f"[cross_shared] max |alpha(1) - alpha(0)| = {(out[1] - out[0]).abs().max().item():.3e}")
    assert counts[1].get("cross_patch_planes", 0) == 1 and counts[0].get("cross_patch_planes", 0) == 0, (counts[1], counts[0])
    assert counts[0]["transpose_v"] - counts[1]["transpose_v"] == N_TRANSFORMER_BLOCKS, (counts[1], counts[0])
    assert counts[0]["conv3x3_thin"] - counts[1]["conv3x3_thin"] == N_TRANSFORMER_BLOCKS, (counts[1], counts[0])


def test_rectangle_shared_and_per_block_forms(eng, engine_option):
    data = _data(1, 128, 256, 10)
    out = {}
    for opt in (1, 0):
        engine_option(eng, "cross_shared", opt)
        out[opt] = _forward(eng, data)
        assert out[opt].shape == (1, 1, 128, 256) and bool(torch.isfinite(out[opt]).all())
        assert out[opt].min().item() >= 0.0 and out[opt].max().item() <= 1.0
    print(f"\n[cross_shared, tiny 128x256] max |alpha(1) - alpha(0)| = {(out[1] - out[0]).abs().max().item():.3e}")
