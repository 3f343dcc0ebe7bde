"""Patch token order of the U-Net transformers (engine option attn_patch_tokens) on the kernel emulator: the helper pair, the way in
(GroupNorm -> operand planes), the way out (the proj_out epilogue of the plane-fed GEMM), and the token-order key bias with its tile list.
(The smallest forward with a patch-order level is 64 x 512 pixels - three minutes on the emulator - so the end-to-end checks are the GPU's:
tests/test_gpu_patch_tokens.py.)"""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patch_tokens_suite as PT  # noqa: E402

DEV = "cpu"


@pytest.fixture(scope="module")
def emu_engine(pkg):
    from emu.build_emu import build
    from comfyui_sdmatte_amd.engine import Bindings, Engine
    from comfyui_sdmatte_amd.config import SDMatteConfig
    eng = Engine(SDMatteConfig.tiny(), 0, True, _lib=Bindings(ctypes.CDLL(build())))
    yield eng
    eng.close()


def test_token_map_is_a_bijection_and_equals_numpy(emu_engine):
    PT.check_map(emu_engine)


def test_way_in_planes_are_the_row_major_rows_permuted(emu_engine):
    PT.check_way_in(emu_engine, DEV)


@pytest.mark.parametrize("mode", [0, 4])
@pytest.mark.parametrize("shape", [(8, 64), (24, 72)])
@pytest.mark.parametrize("O", [32, 160])
def test_way_out_rows_residual_statistics_borders(emu_engine, engine_option, mode, shape, O):
    """256-row tiles: two per image at 8 x 64, a ragged last one (192 rows) at 24 x 72."""
    engine_option(emu_engine, "gemm_p3_tile", 256)
    PT.check_way_out(emu_engine, DEV, mode, shape, O)


@pytest.mark.parametrize("tile,persist", [(128, 1), (64, 8)])
def test_way_out_other_row_tiles(emu_engine, engine_option, tile, persist):
    """The 128- and 64-row tiles, the latter on a persistent grid of 8 blocks that walk several tiles each."""
    engine_option(emu_engine, "gemm_p3_tile", tile)
    engine_option(emu_engine, "gemm_p3_persist", persist)
    PT.check_way_out(emu_engine, DEV, 4, (24, 72), 160)


def test_bias_in_token_order_and_its_tile_list(emu_engine):
    PT.check_bias_and_list(emu_engine, DEV)
