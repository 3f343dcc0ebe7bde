"""Operator checks on checkpoint-like data - large channel means, outlier channels and weights, skewed and mostly constant activations - on the CPU: the real
kernel sources on the fiber emulator.  The cases are realdata_suite.py's; tests/test_gpu_realdata.py runs the same ones on the MI355X."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import realdata_suite  # noqa: E402
from realdata_suite import *  # noqa: E402,F401,F403  (the test functions)


@pytest.fixture(scope="module")
def eng(pkg):
    from emu.build_emu import build
    from comfyui_sdmatte_amd.engine import Bindings, Engine
    from comfyui_sdmatte_amd.config import SDMatteConfig
    e = Engine(SDMatteConfig.tiny(), 0, True, _lib=Bindings(ctypes.CDLL(build())))
    yield e
    e.close()
    realdata_suite.summary("emulator")


@pytest.fixture
def dev():
    return "cpu"


@pytest.fixture
def make_engine(eng):
    from comfyui_sdmatte_amd.engine import Engine
    from comfyui_sdmatte_amd.config import SDMatteConfig
    return lambda: Engine(SDMatteConfig.tiny(), 0, True, _lib=eng.lib)
