"""-m gpu: up-sampling convs as four 2x2-tap phase convs on pre-split operand planes (csrc/k_gemm.h, UP) against the fp32 reference of the layer."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import up_phase_suite as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def eng(pkg):
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.config import SDMatteConfig
    e = Engine(SDMatteConfig.tiny(), 0, True)
    yield e
    e.close()


@pytest.mark.parametrize("i", [0, 1, 2])
def test_up_phase_conv_shapes(eng, engine_option, i):
    engine_option(eng, "conv_up_phase", 2)
    err, _ = U.check_case(eng, DEV, U.SHAPES[i], 10 + i)
    print(f"[up-phase {U.SHAPES[i]}] max|d| = {err:.3e}")


@pytest.mark.parametrize("tile,persist", [(256, 1), (128, 1), (64, 8)])
def test_up_phase_conv_every_row_tile(eng, engine_option, tile, persist):
    engine_option(eng, "conv_up_phase", 2)
    engine_option(eng, "gemm_p3_tile", tile)
    engine_option(eng, "gemm_p3_persist", persist)
    U.check_case(eng, DEV, U.SHAPES[0], 30)


def test_up_phase_conv_model_sized_layer(eng):
    """512 -> 512 at 64 x 64 -> 128 x 128, two images, options at their defaults: 576 tiles of 256 rows, more than one round of resident blocks, so the
    launch takes the phase path by its size; 64 K-loop steps."""
    U.check_case(eng, DEV, (2, 64, 64, 512, 512), 40)


def test_up_phase_statistics(eng, engine_option):
    engine_option(eng, "conv_up_phase", 2)
    U.check_stats(eng, DEV)
    U.check_stats(eng, DEV, shape=(2, 30, 34, 64, 128), seed=6)          # several row tiles per image


def test_up_phase_result_is_the_same_from_run_to_run(eng, engine_option):
    engine_option(eng, "conv_up_phase", 2)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 30, 34, 64, generator=g).cuda()
    w = (torch.randn(128, 64, 3, 3, generator=g) / 24.0).cuda()
    a, sa = eng.op_conv_up_stats(x, w)
    b, sb = eng.op_conv_up_stats(x, w)
    assert torch.equal(a, b) and torch.equal(sa, sb)


def test_up_phase_option_off_keeps_the_3x3_path(eng, engine_option):
    U.check_option_off(eng, DEV, engine_option)


def test_up_phase_model_launch_counts(pkg, engine_option):
    """The model's six Upsample2D layers: all on the phase path with conv_up_phase = 2, none with 0 (read when the engine is built) - and none by
    launch size (1) in this tiny graph at 128 pixels; the alphas agree to the parity bar."""
    from comfyui_sdmatte_amd.engine import Engine, load_library
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.weights import synthetic_state_dict
    from comfyui_sdmatte_amd.synth import synthetic_inputs
    cfg = SDMatteConfig.tiny()
    w = synthetic_state_dict(cfg, 0)
    img, tri = synthetic_inputs(1, 96, 80)
    res = {}
    for o in (2, 1, 0):
        engine_option(load_library(), "conv_up_phase", o)
        e = Engine(cfg, 0, True)
        e.load_state_dict(w)
        e.lib.kernel_counts(reset=True)
        res[o] = (e.apply_matte(img.cuda(), tri.cuda(), 128).cpu(), e.lib.kernel_counts())
        e.close()
    assert res[2][1].get("conv_up_phase", 0) == 6 and res[0][1].get("conv_up_phase", 0) == 0, (res[2][1], res[0][1])
    assert res[1][1] == res[0][1] and torch.equal(res[1][0], res[0][0])
    assert (res[2][0] - res[0][0]).abs().max().item() <= 1e-3


def test_up_phase_output_image_beyond_2gb(eng, engine_option):
    """One output image of 3.2 GB (32 -> 512 channels at 512 x 768 -> 1024 x 1536): a buffer descriptor of 2 GB or more would take the offset that marks a
    dropped store for a valid one, so the epilogue's descriptor spans the tile's own output rows only.  Border rows must not be stored anywhere: the
    result is the same from run to run and agrees with the 3x3 kernels on the up-sampled image (both within 3e-4 of the fp32 reference)."""
    N, H, W, Cin, Cout = 1, 512, 768, 32, 512
    assert 4 * H * W * Cout * 4 > 0x7FFFFFF0
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(N, H, W, Cin, generator=g, device="cuda")
    w = torch.randn(Cout, Cin, 3, 3, generator=g, device="cuda") / (3 * Cin ** 0.5)
    eng.lib.kernel_counts(reset=True)
    a, sa = eng.op_conv_up_stats(x, w)
    b, sb = eng.op_conv_up_stats(x, w)
    assert eng.lib.kernel_counts().get("conv_up_phase", 0) == 2, eng.lib.kernel_counts()
    assert torch.equal(a, b) and torch.equal(sa, sb)
    del b, sb
    engine_option(eng, "conv_up_phase", 0)
    r, _ = eng.op_conv_up_stats(x, w)
    assert eng.lib.kernel_counts().get("conv_up_phase", 0) == 2
    assert (a - r).abs().max().item() < 6e-4
