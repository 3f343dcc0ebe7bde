"""-m gpu: patch token order of the U-Net transformers (engine option attn_patch_tokens): the helper pair, the way in, the way out, the
token-order key bias with its tile list, and the tiny architecture end to end at 512 x 512 (level 0 = 64 x 64 in patch order, level 1 = 32 x 32 row-major)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patch_tokens_suite as PT  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3


@pytest.fixture(scope="module")
def eng(pkg):
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.config import SDMatteConfig
    e = Engine(SDMatteConfig.tiny(), 0, True)
    yield e
    e.close()


def test_token_map_is_a_bijection_and_equals_numpy(eng):
    PT.check_map(eng)


def test_way_in_planes_are_the_row_major_rows_permuted(eng):
    PT.check_way_in(eng, DEV)


@pytest.mark.parametrize("mode", [0, 4])
@pytest.mark.parametrize("shape", [(8, 64), (24, 72)])
@pytest.mark.parametrize("O", [32, 160])
def test_way_out_rows_residual_statistics_borders(eng, engine_option, mode, shape, O):
    """256-row tiles: two per image at 8 x 64, a ragged last one (192 rows) at 24 x 72."""
    engine_option(eng, "gemm_p3_tile", 256)
    PT.check_way_out(eng, DEV, mode, shape, O)


@pytest.mark.parametrize("tile,persist", [(0, 1), (128, 1), (64, 8)])
def test_way_out_other_row_tiles(eng, engine_option, tile, persist):
    """The row tile the launcher picks by itself, the 128- and 64-row tiles, the latter on a persistent grid of 8 blocks that walk several tiles each."""
    engine_option(eng, "gemm_p3_tile", tile)
    engine_option(eng, "gemm_p3_persist", persist)
    PT.check_way_out(eng, DEV, 4, (24, 72), 160)


def test_bias_in_token_order_and_its_tile_list(eng):
    PT.check_bias_and_list(eng, DEV)


@pytest.fixture(scope="module")
def tiny_model(pkg):
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.weights import synthetic_state_dict
    cfg = SDMatteConfig.tiny()
    w = synthetic_state_dict(cfg, 0)
    e = Engine(cfg, 0)
    e.load_state_dict(w)
    yield cfg, w, e
    e.close()


def test_e2e_tiny_512_both_orders_vs_oracle(tiny_model, engine_option):
    """S = 512, B = 2: both token orders within TOL of the oracle; with the option on the dense walk is bit-identical to the tile-skipping one; the launch
    counter shows proj_out's mapped instantiation for the five transformers of level 0 and for no other."""
    from comfyui_sdmatte_amd.synth import synthetic_inputs
    from oracle import sdmatte_oracle as O
    cfg, w, e = tiny_model
    S = 512
    img, tri = synthetic_inputs(2, S, S, seed=1234)
    data = O.preprocess(img, tri, S, False)
    ref = O.sdmatte_forward(w, cfg.as_dict(), data)
    out = {}
    for opt in (1, 0):
        engine_option(e, "attn_patch_tokens", opt)
        e.lib.kernel_counts(reset=True)
        out[opt] = e.forward(data["image"].cuda(), data["trimap"].cuda(), is_trans=data["is_trans"].numpy()).cpu()
        c = e.lib.kernel_counts()
        assert c.get("gemm_p3_tokens", 0) == (5 if opt else 0), (opt, c)
        d = (out[opt] - ref).abs().max().item()
        print(f"[patch tokens] tiny S=512 B=2, attn_patch_tokens = {opt}: max |alpha - oracle| = {d:.3e}")
        assert d <= TOL, (opt, d)
    print(f"[patch tokens] tiny S=512 B=2: max |alpha(1) - alpha(0)| = {(out[1] - out[0]).abs().max().item():.3e}")
    engine_option(e, "attn_patch_tokens", 1)
    engine_option(e, "attn_dense", 1)
    dense = e.forward(data["image"].cuda(), data["trimap"].cuda(), is_trans=data["is_trans"].numpy()).cpu()
    assert torch.equal(dense, out[1])


def test_e2e_rectangle_that_fails_the_rule_is_bit_identical(tiny_model, engine_option):
    """128 x 448 pixels: level 0 is a 16 x 56 latent, narrower than 64, so every level keeps row-major order: the option moves no bit and the mapped
    instantiation never runs."""
    from comfyui_sdmatte_amd.synth import synthetic_inputs
    cfg, w, e = tiny_model
    img, tri = synthetic_inputs(2, 128, 448, seed=8)
    image, trimap = ((img.permute(0, 3, 1, 2).contiguous() - 0.5) / 0.5).cuda(), (tri.unsqueeze(1) * 2 - 1).cuda()
    out = {}
    for opt in (1, 0):
        engine_option(e, "attn_patch_tokens", opt)
        e.lib.kernel_counts(reset=True)
        out[opt] = e.forward(image, trimap, is_trans=[0, 1]).cpu()
        assert e.lib.kernel_counts().get("gemm_p3_tokens", 0) == 0
    assert torch.equal(out[1], out[0])
