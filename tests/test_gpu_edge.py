"""The distance field and its two consumers on the MI355X (csrc/k_distance.h through sdm_distance_field / sdm_offset_mask / sdm_outline): the field exact
against the references of tests/edge_suite.py and against the existing trimap kernels, the consumers against the fp64 restatement.  No weights are loaded."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def bare_engine(pkg):
    """An engine that never loads weights: the three calls need none."""
    from comfyui_sdmatte_amd.config import SDMatteConfig
    from comfyui_sdmatte_amd.engine import Engine
    eng = Engine(SDMatteConfig.tiny(), 0)
    yield eng
    eng.close()


def test_gpu_distance_field_equals_brute_force(bare_engine):
    import edge_suite as ES
    ES.check_field(bare_engine, lambda t: t.cuda(), ES.field_cases("brute"))
    ES.check_field(bare_engine, lambda t: t, ES.field_cases("brute"))


def test_gpu_distance_field_equals_restatement_device_pointers(bare_engine):
    import edge_suite as ES
    ES.check_field(bare_engine, lambda t: t.cuda(), ES.field_cases("restatement"))


def test_gpu_distance_field_equals_restatement_host_pointers(bare_engine):
    import edge_suite as ES
    ES.check_field(bare_engine, lambda t: t, ES.field_cases("restatement"))


def test_gpu_distance_field_batch_and_misaligned_device_pointer(bare_engine):
    import edge_suite as ES
    import roi_suite as RS
    ES.check_field_batch(bare_engine, lambda t: t.cuda())
    ES.check_field_batch(bare_engine, lambda t: RS.misaligned(t.cuda()))
    ES.check_field(bare_engine, lambda t: RS.misaligned(t.cuda()), [c for c in ES.field_cases("restatement") if c[0].endswith(("96x128", "130x257"))])


@pytest.mark.parametrize("size", [(540, 960), (1080, 1920)], ids=["540x960", "1080x1920"])
def test_gpu_distance_field_seeds_closed_form(bare_engine, size):
    """50 seed pixels per image, B = 2, and the complement (everything foreground but 50 holes)."""
    import edge_suite as ES
    plane, field = ES.seed_case(*size)
    assert int((field == 1).sum()) >= 8 and int((field == 2).sum()) >= 2      # isolated seeds, and the centre of a clump in either image
    assert np.array_equal(bare_engine.distance_field(torch.from_numpy(plane).cuda()).cpu().numpy(), field)
    assert np.array_equal(bare_engine.distance_field(torch.from_numpy(1.0 - plane).cuda()).cpu().numpy(), -field)


def test_gpu_distance_field_one_seed_in_a_row_of_32768(bare_engine):
    import edge_suite as ES
    plane, field = ES.long_row_case()
    assert np.array_equal(bare_engine.distance_field(torch.from_numpy(plane).cuda()).cpu().numpy(), field)
    assert np.array_equal(bare_engine.distance_field(torch.from_numpy(plane)).numpy(), field)
    col = torch.from_numpy(plane.reshape(1, -1, 1).copy()).cuda()               # ... and in a column of 32768: 1024 tiles
    assert np.array_equal(bare_engine.distance_field(col).cpu().numpy(), field.reshape(1, -1, 1))


def test_gpu_distance_field_on_a_side_stream(bare_engine):
    """The plane is produced on a side stream right before the call and the field consumed on it right after: the engine orders itself on both ends."""
    import edge_suite as ES
    plane, want = ES.batch_case()
    base = torch.from_numpy(plane).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        p = base * 1.0
        field = bare_engine.distance_field(p, 0.5, sync=False)
        doubled = field.long() * 2
    st.synchronize()
    assert np.array_equal(doubled.cpu().numpy(), want.astype(np.int64) * 2)


@pytest.mark.parametrize("size", [(300, 500), (1080, 1920)], ids=["300x500", "1080x1920"])
def test_gpu_distance_field_against_trimap_kernels(bare_engine, size):
    import edge_suite as ES
    ES.check_field_against_trimap(bare_engine, lambda t: t.cuda(), *size, ((0, 0), (1, 2), (10, 10), (255, 255)))


def test_gpu_offset_mask(bare_engine):
    import edge_suite as ES
    ES.check_offset_mask(bare_engine, lambda t: t.cuda())
    ES.check_offset_mask(bare_engine, lambda t: t)
    ES.check_offset_mask_exact_consequences(bare_engine, lambda t: t.cuda())


def test_gpu_outline(bare_engine):
    import edge_suite as ES
    ES.check_outline(bare_engine, lambda t: t.cuda())
    ES.check_outline(bare_engine, lambda t: t)
    ES.check_outline_exact_properties(bare_engine, lambda t: t.cuda())


def test_gpu_edge_argument_checks(bare_engine):
    import edge_suite as ES
    ES.check_errors(bare_engine, lambda t: t.cuda())
    ES.check_errors(bare_engine, lambda t: t)


def test_gpu_edge_memory_is_counted_and_released(bare_engine):
    import edge_suite as ES
    ES.check_memory(bare_engine, lambda t: t.cuda())
    ES.check_memory(bare_engine, lambda t: t)


@pytest.mark.parametrize("case", ["blobs_B2_96x128", "corner_pixel_B1_130x257"])
def test_gpu_edge_profile_shows_each_launch_once(bare_engine, case):
    """Two sizes and contents: every documented launch exactly once per call in the per-launch profile, and a call time."""
    import edge_suite as ES
    if case.startswith("blobs"):
        fg, alpha = ES.outline_inputs(96, 128, 2)
    else:
        alpha = torch.from_numpy(dict((n, p) for n, p, _ in ES.contents(130, 257))["corner_pixel"][None])
        fg = torch.rand(1, 130, 257, 3)
    fg, alpha = fg.cuda(), alpha.cuda()
    for kind, call in (("field", lambda: bare_engine.distance_field(alpha)), ("offset", lambda: bare_engine.offset_mask(alpha, 5.0, 2.0)),
                       ("outline", lambda: bare_engine.outline(fg, alpha, 4.0))):
        bare_engine.profile(True)
        call()
        bare_engine.profile(False)
        res = bare_engine.profile_results()
        assert {k: res[k]["launches"] for k in res} == {k: 1 for k in ES.DF_KERNELS[kind]}, (kind, sorted(res))
        dump = bare_engine.profile_dump()
        assert all(dump.count(k + ",") == 1 for k in ES.DF_KERNELS[kind]), kind
        assert bare_engine.last_forward_ms() > 0.0
