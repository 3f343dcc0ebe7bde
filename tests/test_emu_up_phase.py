"""Up-sampling convs as four 2x2-tap phase convs on pre-split operand planes (csrc/k_gemm.h, UP), on the CPU: the phase-weight algebra in float64 and the
real kernel sources - weight derivation, bordered-plane pre-pass, GEMM variant - on the fiber emulator."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import up_phase_suite as U  # noqa: E402

DEV = "cpu"


@pytest.fixture(scope="module")
def emu_engine(pkg):
    from emu.build_emu import build
    from comfyui_sdmatte_amd.engine import Bindings, Engine
    from comfyui_sdmatte_amd.config import SDMatteConfig
    eng = Engine(SDMatteConfig.tiny(), 0, True, _lib=Bindings(ctypes.CDLL(build())))
    yield eng
    eng.close()


def test_phase_weights_equal_upsample_conv3x3_float64(pkg):
    """Four 2x2 convs with the summed taps == nearest x2 + conv3x3 (zero padding included), to 1e-12 in float64."""
    from comfyui_sdmatte_amd.weights import up_phase_weights
    g = torch.Generator().manual_seed(0)
    for (N, H, W, I, O) in [(2, 5, 7, 6, 4), (1, 1, 1, 3, 2), (1, 2, 9, 5, 7)]:
        x = torch.randn(N, I, H, W, generator=g, dtype=torch.float64)
        w = torch.randn(O, I, 3, 3, generator=g, dtype=torch.float64)
        ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, padding=1)
        w2 = up_phase_weights(w)
        xp = F.pad(x, (1, 1, 1, 1))
        got = torch.zeros_like(ref)
        for py in range(2):
            for px in range(2):
                # tap (a, b) reads source pixel (y + py - 1 + a, x + px - 1 + b) = bordered pixel (y + py + a, x + px + b)
                full = F.conv2d(xp, w2[py, px])                          # [N, O, H + 1, W + 1]: window origin (y', x') covers bordered rows y' .. y' + 1
                got[:, :, py::2, px::2] = full[:, :, py:py + H, px:px + W]
        assert (got - ref).abs().max().item() < 1e-12


@pytest.mark.parametrize("i", [0, 1, 2])
def test_up_phase_conv_shapes(emu_engine, engine_option, i):
    engine_option(emu_engine, "conv_up_phase", 2)
    err, _ = U.check_case(emu_engine, DEV, U.SHAPES[i], 10 + i)
    print(f"[up-phase {U.SHAPES[i]}] max|d| = {err:.3e}")


@pytest.mark.parametrize("tile,persist", [(256, 1), (128, 1), (64, 8)])
def test_up_phase_conv_every_row_tile(emu_engine, engine_option, tile, persist):
    """The 256- and 128-row tiles (ragged: an image of 63 bordered rows), and a persistent grid of 8 blocks that walk several (tile, phase) pairs each."""
    engine_option(emu_engine, "conv_up_phase", 2)
    engine_option(emu_engine, "gemm_p3_tile", tile)
    engine_option(emu_engine, "gemm_p3_persist", persist)
    U.check_case(emu_engine, DEV, U.SHAPES[0], 30)


def test_up_phase_statistics(emu_engine, engine_option):
    engine_option(emu_engine, "conv_up_phase", 2)
    U.check_stats(emu_engine, DEV)


def test_up_phase_option_off_keeps_the_3x3_path(emu_engine, engine_option):
    U.check_option_off(emu_engine, DEV, engine_option)
