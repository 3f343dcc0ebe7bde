"""The GroupNorm statistics chain - conv / GEMM epilogue partial rows, gn_partials_scale_shift_kernel, fused-GroupNorm consumer - on the CPU: the real
kernel sources on the fiber emulator (gn_chain_suite.py).  The F8 kernel's register-direct epilogue adds its rows with a helper here, with DPP row adds on
hardware: tests/test_gpu_gn_chain.py runs the same cases there."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gn_chain_suite as G  # noqa: E402

DEV = "cpu"


@pytest.fixture(scope="module")
def emu_engine(pkg):
    from emu.build_emu import build
    from comfyui_sdmatte_amd.engine import Bindings, Engine
    from comfyui_sdmatte_amd.config import SDMatteConfig
    eng = Engine(SDMatteConfig.tiny(), 0, True, _lib=Bindings(ctypes.CDLL(build())))
    yield eng
    eng.close()


@pytest.mark.parametrize("name", list(G.PRODUCERS))
def test_partial_rows_are_the_sums_of_the_stored_output(emu_engine, engine_option, name):
    G.check_partials(emu_engine, DEV, engine_option, name)


def test_partial_rows_of_constant_tiles(emu_engine, engine_option):
    G.check_const_tiles(emu_engine, DEV, engine_option)


@pytest.mark.parametrize("name", list(G.REDUCERS))
def test_reducer_against_float64(emu_engine, name):
    G.check_reducer(emu_engine, DEV, name)


@pytest.mark.parametrize("name", list(G.CHAINS))
def test_producer_reducer_consumer(emu_engine, engine_option, name):
    G.check_chain(emu_engine, DEV, engine_option, name)


def test_error_over_bound_per_family(emu_engine):
    """(after the cases above) the largest statistics error / bound per producer family, for profiles/NOTES.md"""
    for fam, (e1, e2) in sorted(G.RATIOS.items()):
        print(f"[gn chain / emulator] {fam}: sum {e1:.3f}, sum of squares {e2:.3f}")
        assert e1 <= 1.0 and e2 <= 1.0


def test_hooks_size_their_arena_on_a_fresh_engine(emu_engine, engine_option):
    """sdm_op_conv_stats (with input statistics and with the poison on) and sdm_op_gn_partials on an engine whose arena has never grown: the sizing pass
    and the launch pass allocate alike, or the arena check fails the call (test_emu_ops.test_arena_check_self_test)."""
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.config import SDMatteConfig
    eng = Engine(SDMatteConfig.tiny(), 0, True, _lib=emu_engine.lib)
    try:
        G.check_chain(eng, DEV, engine_option, "concat_cfg0_f8")
        G.check_reducer(eng, DEV, "straddle_vec2")
        G.check_partials(eng, DEV, engine_option, "splitk_1x1_k2_f16_res")
    finally:
        eng.close()


def test_poison_option_is_off_by_default_and_changes_nothing_but_unwritten_rows(emu_engine, engine_option):
    """dbg_stats_poison = 0 is the default; with it on, output and statistics of a launch that writes all its rows are bit-identical."""
    assert emu_engine.lib.get_option("dbg_stats_poison") == 0
    g = torch.Generator().manual_seed(9)
    x, w = torch.randn(2, 12, 40, 64, generator=g), torch.randn(160, 64, 3, 3, generator=g) / 24.0
    kw = dict(tile_cfg=0, split=True, out_f32=True)
    a, sa = emu_engine.op_conv_stats(x, w, **kw)
    engine_option(emu_engine, "dbg_stats_poison", 1)
    b, sb = emu_engine.op_conv_stats(x, w, **kw)
    assert torch.equal(a, b) and torch.equal(sa[..., :160, :], sb[..., :160, :])
