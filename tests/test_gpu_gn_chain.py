"""-m gpu: the GroupNorm statistics chain - conv / GEMM epilogue partial rows, gn_partials_scale_shift_kernel, fused-GroupNorm consumer - on the MI355X
(gn_chain_suite.py).  The F8 3x3 kernel's register-direct epilogue adds its rows with DPP row adds that only hardware runs."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gn_chain_suite as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def eng(pkg):
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.config import SDMatteConfig
    e = Engine(SDMatteConfig.tiny(), 0, True)
    yield e
    e.close()


@pytest.mark.parametrize("name", list(G.PRODUCERS))
def test_partial_rows_are_the_sums_of_the_stored_output(eng, engine_option, name):
    G.check_partials(eng, DEV, engine_option, name)


def test_partial_rows_of_constant_tiles(eng, engine_option):
    G.check_const_tiles(eng, DEV, engine_option)


@pytest.mark.parametrize("name", list(G.REDUCERS))
def test_reducer_against_float64(eng, name):
    G.check_reducer(eng, DEV, name)


@pytest.mark.parametrize("name", list(G.CHAINS))
def test_producer_reducer_consumer(eng, engine_option, name):
    G.check_chain(eng, DEV, engine_option, name)


def test_error_over_bound_per_family(eng):
    """(after the cases above) the largest statistics error / bound per producer family, for profiles/NOTES.md"""
    for fam, (e1, e2) in sorted(G.RATIOS.items()):
        print(f"[gn chain / MI355X] {fam}: sum {e1:.3f}, sum of squares {e2:.3f}")
        assert e1 <= 1.0 and e2 <= 1.0
