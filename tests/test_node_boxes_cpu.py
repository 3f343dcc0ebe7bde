"""A box per subject on the CPU: sdmatte_nodes.subject_boxes against the brute force of tests/boxes_suite.py, paste_boxes, compact_boxes, the opt-in node
SDMatteApplySubjects with its splitting rule against a stub engine, and the mappings.  No GPU, no emulator."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def test_subject_boxes_restatement_equals_brute_force(pkg):
    import boxes_suite as BS
    from comfyui_sdmatte_amd.sdmatte_nodes import subject_boxes, subject_roi
    for name, plane, thr, ma, K, mpx, mpct, sq in BS.box_cases():
        got, cnt = subject_boxes(torch.from_numpy(plane), thr, ma, K, mpx, mpct, sq, return_count=True)
        want, wcnt = BS.brute_force(plane, thr, ma, K, mpx, mpct, sq)
        assert got.dtype == torch.int32 and cnt.dtype == torch.int32 and np.array_equal(got.numpy(), want) and np.array_equal(cnt.numpy(), wcnt), name
        assert BS.covered(plane, thr, want), name
        one = subject_boxes(torch.from_numpy(plane), thr, ma, 1, mpx, mpct, sq)
        assert torch.equal(one[:, 0, 1:], subject_roi(torch.from_numpy(plane), thr, mpx, mpct, sq)), name


def test_subject_boxes_cases_mean_what_their_names_say(pkg):
    import boxes_suite as BS
    cases = {c[0]: c for c in BS.box_cases()}
    assert len(cases) == len(BS.box_cases())

    def run(name):
        _, plane, thr, ma, K, mpx, mpct, sq = cases[name]
        b, c = BS.brute_force(plane, thr, ma, K, mpx, mpct, sq)
        return b[0, :c[0], 1:].tolist()
    assert [len(run(f"three_blobs_K{K}")) for K in (1, 2, 3, 4, 8)] == [1, 2, 3, 3, 3]
    assert run("three_blobs_K2")[0] == run("three_blobs_K8")[0] and run("three_blobs_K2")[1] != run("three_blobs_K8")[1]      # the rest box of two blobs
    assert run("area_tie_smaller_root_wins")[0] == [9, 9, 22, 12]                                                       # the blob at (10, 10), not (60, 80)
    assert len(run("min_area_at_the_area")) == len(run("min_area_below_the_area")) == 4 and len(run("min_area_above_the_area")) == 3
    assert len(run("small_inside_margin_box_dropped")) == 1 and len(run("small_one_pixel_outside_kept")) == 2
    assert run("small_one_pixel_outside_kept")[1] != run("small_one_pixel_outside_to_rest")[1]
    assert run("speckle_gives_the_rest_box")[2] == [0, 0, 97, 131]
    assert len(run("more_candidates_than_slots")) == 4 and len(run("more_candidates_than_slots_K8_square")) == 8
    assert run("empty") == run("empty_at_threshold") == run("whole_frame") == [[0, 0, 97, 131]]
    assert run("nan_is_outside")[0] == [38, 48, 24, 44]
    assert run("diagonal_lines_are_connected") == [[10, 41, 60, 60], [5, 5, 35, 35]]
    e = run("edges_margins_clip")
    assert any(b[0] == 0 for b in e) and any(b[1] == 0 for b in e) and any(b[0] + b[2] == 97 for b in e) and any(b[1] + b[3] == 131 for b in e)
    assert all(b[2] == b[3] for b in run("edges_square_shifts"))


def test_subject_boxes_argument_checks(pkg):
    from comfyui_sdmatte_amd.sdmatte_nodes import subject_boxes
    p = torch.rand(1, 6, 7)
    for bad in ({"roi_threshold": 1.0}, {"margin_px": 4097}, {"margin_pct": 101}, {"min_area": -1}, {"min_area": 2.5}, {"max_boxes": 0}, {"max_boxes": 9}):
        with pytest.raises(ValueError):
            subject_boxes(p, **bad)
    with pytest.raises(ValueError):
        subject_boxes(p[0])
    assert subject_boxes(torch.zeros(1, 6, 7)).tolist() == [[[0, 0, 0, 6, 7]] + [[-1, 0, 0, 0, 0]] * 3]


def test_paste_and_compact_boxes(pkg):
    from comfyui_sdmatte_amd.sdmatte_nodes import compact_boxes, paste_boxes
    crops = [torch.full((3, 4), 0.5), torch.full((3, 4), 0.25), torch.full((2, 2), 0.75), torch.full((1, 1), 9.0)]
    boxes = torch.tensor([[0, 1, 1, 3, 4], [0, 2, 3, 3, 4], [1, 0, 0, 2, 2], [-1, 0, 0, 0, 0]], dtype=torch.int32)
    out = paste_boxes(crops, boxes, 2, 6, 8)
    assert out.shape == (2, 6, 8) and out.dtype == torch.float32
    want = torch.zeros(2, 6, 8)
    want[0, 2:5, 3:7] = 0.25
    want[0, 1:4, 1:5] = 0.5                                                                   # the maximum where the two meet
    want[1, 0:2, 0:2] = 0.75
    assert torch.equal(out, want)
    for bad in ((crops[:3], boxes), (crops, torch.tensor([[0, 1, 1, 3, 4], [0, 4, 3, 3, 4], [1, 0, 0, 2, 2], [-1, 0, 0, 0, 0]])),
                (crops, torch.tensor([[2, 1, 1, 3, 4], [0, 2, 3, 3, 4], [1, 0, 0, 2, 2], [-1, 0, 0, 0, 0]]))):
        with pytest.raises(ValueError):
            paste_boxes(bad[0], bad[1], 2, 6, 8)
    c = compact_boxes(boxes.reshape(2, 2, 5))
    assert c.dtype == torch.int32 and c.tolist() == boxes[:3].tolist() and compact_boxes(boxes[3:]).shape == (0, 5)


class _StubEngine:
    """Records the apply_matte_boxes calls; make_trimap and subject_boxes are the CPU restatements."""
    BOXES_MAX_TOTAL = 16

    def __init__(self):
        self.calls = []

    def make_trimap(self, mask, threshold, erode_px, dilate_px):
        from comfyui_sdmatte_amd.sdmatte_nodes import trimap_from_mask
        return trimap_from_mask(mask, threshold, erode_px, dilate_px)

    def subject_boxes(self, plane, *args):
        from comfyui_sdmatte_amd.sdmatte_nodes import subject_boxes
        return subject_boxes(plane, *args)

    def apply_matte_boxes(self, image, trimap, boxes, S, is_transparent, output_mode, mask_refine, trimap_constraint):
        self.calls.append((tuple(image.shape), boxes.clone()))
        B, H, W, _ = image.shape
        assert boxes.dtype == torch.int32 and 1 <= boxes.shape[0] <= 16 and int(boxes[:, 0].min()) >= 0 and int(boxes[:, 0].max()) < B
        return torch.full((B, H, W), float(len(self.calls))), torch.zeros(B, H, W, 3)


def test_subjects_node_splits_the_batch(pkg, monkeypatch):
    """B = 5 images with three blobs each and max_subjects = 8: 3 boxes per image, 15 in all -> one call; with a speck each 4 per image, 20 in all -> the calls
    get 4 + 1 images (16 + 4 entries), b rebased; the outputs come back in image order."""
    import boxes_suite as BS
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    monkeypatch.setattr(N, "_trim_engine_memory", lambda model: None)
    monkeypatch.delenv("SDMATTE_MULTI_GPU", raising=False)

    class Model:
        pass
    for rects, per_image, want_calls in ((BS.THREE, 3, [(0, 5)]), (BS.THREE + ((2, 4, 120, 123), ), 4, [(0, 4), (4, 5)])):
        model = Model()
        model.engine = _StubEngine()
        mask = torch.from_numpy(BS.paint(97, 131, rects, B=5))
        image = torch.rand(5, 97, 131, 3)
        a, m, t, boxes = N.SDMatteApplySubjects._run(model, image, mask, 0.5, 0, 0, 0.0, 2, 5, False, 8, 64, 64, False, "alpha_only", False, 0.8)
        assert [c[0][0] for c in model.engine.calls] == [hi - lo for lo, hi in want_calls]
        for (lo, hi), (_, part) in zip(want_calls, model.engine.calls):
            assert part.shape[0] == per_image * (hi - lo) <= 16 and sorted(set(part[:, 0].tolist())) == list(range(hi - lo))
        assert a.shape == (5, 97, 131) and m.shape == (5, 97, 131, 3) and torch.equal(t, mask)
        assert [float(a[b, 0, 0]) for b in range(5)] == [float(i + 1) for i, (lo, hi) in enumerate(want_calls) for _ in range(lo, hi)]
        assert len(boxes) == 5 and all(len(bx) == per_image for bx in boxes)
        want, _ = BS.brute_force(mask.numpy(), 0.0, 64, 8, 2, 5, False)
        assert boxes[3] == [(x0, y0, w, h) for _, y0, x0, h, w in want[3, :per_image].tolist()]


def test_split_boxes(pkg):
    from comfyui_sdmatte_amd.sdmatte_nodes import split_boxes
    boxes = torch.tensor([[b, 0, 0, 1, 1] for b in (0, 0, 0, 2, 2, 3)], dtype=torch.int32)            # image 1 has no box
    assert [(lo, hi, p[:, 0].tolist()) for lo, hi, p in split_boxes(boxes, 4, 16)] == [(0, 4, [0, 0, 0, 2, 2, 3])]
    assert [(lo, hi, p[:, 0].tolist()) for lo, hi, p in split_boxes(boxes, 4, 3)] == [(0, 2, [0, 0, 0]), (2, 4, [0, 0, 1])]
    with pytest.raises(ValueError):
        split_boxes(boxes, 4, 2)


def test_node_mappings_with_subjects(pkg):
    """Every earlier argument combination returns what it returned; subjects=True adds exactly SDMatteApplySubjects."""
    from comfyui_sdmatte_amd import sdmatte_nodes as N
    from comfyui_sdmatte_amd.engine import Engine
    assert inspect.signature(N.node_mappings).parameters["subjects"].default is False
    for args in ((False, ), (True, True, True, True, True, True), (True, False, True, False, True, False)):
        base_c, base_n = N.node_mappings(*args)
        assert "SDMatteApplySubjects" not in base_c and N.node_mappings(*args, subjects=False) == (base_c, base_n)
        classes, names = N.node_mappings(*args, subjects=True)
        assert classes == dict(base_c, SDMatteApplySubjects=N.SDMatteApplySubjects) and names == dict(base_n, SDMatteApplySubjects="Apply SDMatte (Subjects)")
    f = N.SDMatteApplySubjects
    it = f.INPUT_TYPES()
    roi_req = N.SDMatteApplyROI.INPUT_TYPES()["required"]
    new = ["max_subjects", "min_area"]
    assert [k for k in it["required"] if k not in new] == list(roi_req) and all(it["required"][k] == roi_req[k] for k in roi_req)
    assert [k for k in it["required"] if k in new] == new and it["optional"] == N.SDMatteApplyROI.INPUT_TYPES()["optional"]
    req = it["required"]
    defaults = {k: v.default for k, v in inspect.signature(Engine.subject_boxes).parameters.items() if v.default is not inspect.Parameter.empty}
    assert req["max_subjects"][1]["default"] == defaults["max_boxes"] and req["min_area"][1]["default"] == defaults["min_area"]
    assert (req["max_subjects"][0], req["max_subjects"][1]["min"], req["max_subjects"][1]["max"]) == ("INT", 1, Engine.BOXES_MAX)
    assert (req["min_area"][0], req["min_area"][1]["min"], req["min_area"][1]["max"]) == ("INT", 0, Engine.CLEAN_MAX_AREA)
    assert {k: v.default for k, v in inspect.signature(N.subject_boxes).parameters.items() if k in defaults} == {
        k: v for k, v in defaults.items() if k in inspect.signature(N.subject_boxes).parameters}
    assert f.RETURN_TYPES == ("MASK", "IMAGE", "MASK", "BBOX") and len(f.RETURN_NAMES) == 4 and f.CATEGORY == "Matting/SDMatte"
    assert list(inspect.signature(getattr(f, f.FUNCTION)).parameters) == ["self"] + list(req) + list(it["optional"])
    # input validation comes before any model is looked for
    img, msk = torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8)
    tail = (64, False, "alpha_only", True, 0.8)
    for bad in ((img[..., :2], msk, 0.5, 1, 1, 0.0, 1, 1, True, 4, 64), (img, msk[:, :4], 0.5, 1, 1, 0.0, 1, 1, True, 4, 64), (img, msk, 0.5, 1, 1, 1.0, 1, 1, True, 4, 64),
                (img, msk, 0.5, 1, 1, 0.0, 1, 1, True, 9, 64), (img, msk, 0.5, 1, 1, 0.0, 1, 1, True, 0, 64), (img, msk, 0.5, 1, 1, 0.0, 1, 1, True, 4, -1)):
        with pytest.raises(ValueError):
            f().apply_matte("SDMatte.safetensors", *bad, *tail)
    with pytest.raises(RuntimeError):
        f().apply_matte("SDMatte.safetensors", img, msk, 0.5, 1, 1, 0.0, 1, 1, True, 4, 64, *tail, force_cpu=True)


def test_subjects_node_env_opt_in(pkg):
    """The module-level mappings follow SDMATTE_SUBJECTS_NODE, independently of the other flags: a fresh interpreter each."""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; p = load_package(); "
            "print(sorted(p.NODE_CLASS_MAPPINGS), sorted(p.NODE_DISPLAY_NAME_MAPPINGS))" % ROOT)
    flags = ("SDMATTE_EXTRA_NODES", "SDMATTE_FOREGROUND_NODE", "SDMATTE_REFINE_NODE", "SDMATTE_CLEAN_NODE", "SDMATTE_ROI_NODE", "SDMATTE_CANVAS_NODE",
             "SDMATTE_SUBJECTS_NODE")
    for roi, sub, want in ((None, None, "['SDMatteApply']"), (None, "0", "['SDMatteApply']"), (None, "1", "['SDMatteApply', 'SDMatteApplySubjects']"),
                           ("1", "1", "['SDMatteApply', 'SDMatteApplyROI', 'SDMatteApplySubjects']"), ("1", None, "['SDMatteApply', 'SDMatteApplyROI']")):
        env = {k: v for k, v in os.environ.items() if k not in flags}
        env.update({k: v for k, v in (("SDMATTE_ROI_NODE", roi), ("SDMATTE_SUBJECTS_NODE", sub)) if v is not None})
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout.strip() == f"{want} {want}", (roi, sub, r.stdout, r.stderr)


def test_product_library_exports_boxes_calls(pkg):
    """The gfx950 library exports the two new product calls, and header and bindings agree on the limits."""
    from comfyui_sdmatte_amd import build, engine
    dll = ctypes.CDLL(build.build_all())
    for name in ("sdm_subject_boxes", "sdm_apply_matte_boxes"):
        assert name in engine.EXPORTS
        getattr(dll, name)
    hdr = open(os.path.join(ROOT, "include", "sdmatte.h")).read()
    assert f"#define SDM_BOXES_MAX {engine.Engine.BOXES_MAX}\n" in hdr and f"#define SDM_BOXES_MAX_TOTAL {engine.Engine.BOXES_MAX_TOTAL}\n" in hdr
