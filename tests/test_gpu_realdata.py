"""-m gpu: operator checks on checkpoint-like data - large channel means, outlier channels and weights, skewed and mostly constant activations - on the
MI355X.  The cases are realdata_suite.py's (tests/test_emu_realdata.py runs the same ones on the emulator); the reduction orders of the hardware kernels - DPP
row adds in the F8 epilogue, atomics in the stand-alone statistics - exist only here."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import realdata_suite  # noqa: E402
from realdata_suite import *  # noqa: E402,F401,F403  (the test functions)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(pkg):
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.config import SDMatteConfig
    e = Engine(SDMatteConfig.tiny(), 0, True)
    yield e
    e.close()
    realdata_suite.summary("MI355X")


@pytest.fixture
def dev():
    return "cuda"


@pytest.fixture
def make_engine(eng):
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.config import SDMatteConfig
    return lambda: Engine(SDMatteConfig.tiny(), 0, True)
