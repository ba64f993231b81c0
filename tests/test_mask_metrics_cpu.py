"""Mask-level video metrics, the part that needs no GPU: the two entry points of csrc/mask_metrics.hip are declared, exported and
refuse bad arguments before any GPU call; the numpy / scipy restatement of tests/maskmetric_cases.py reproduces what the
reference's executed seg2bmap, db_eval_boundary and db_eval_iou gave on the fixture (tests/golden/video_metrics_tiny.json), bit
for bit and float for float; the radius rule, the window arithmetic of VideoMaskEval and the refusals of the Python side."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from phnet_amd import _lib
from phnet_amd import build as hip_build
from phnet_amd.evaluation import video as V
from tests import maskmetric_cases as C

ERR_ARG = -1


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.SO_PATH):
        hip_build.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------ the entry points
def test_symbols_are_declared_and_exported(built):
    names = {n: a for n, _, a in _lib.declared_functions(_lib.HEADER)}
    assert len(names["phnet_mask_metrics"]) == 10 and len(names["phnet_mask_metrics_workspace"]) == 4
    assert hasattr(built, "phnet_mask_metrics") and hasattr(built, "phnet_mask_metrics_workspace")
    assert built.phnet_abi_version() == 1
    header = open(_lib.HEADER).read()
    for rule in ("a pixel is foreground iff its byte is not 0", "b = (s^e) | (s^so) | (s^se)", "the bottom-right pixel: b = 0",
                 "dx^2 + dy^2 <= radius^2", "PARITY UNPINNED against skimage",
                 "area_pred, area_gt, area_both", "fg_match = |b_pred & dil(b_gt)|, gt_match = |b_gt & dil(b_pred)|"):
        assert rule in header, rule


def test_published_constants_match_the_python_side():
    from phnet_amd import hip_ops
    defines = dict(re.findall(r"#define (PHNET_MASK_METRICS_\w+) (\d+)", open(_lib.HEADER).read()))
    assert int(defines["PHNET_MASK_METRICS_MAX_RADIUS"]) == hip_ops.MASK_METRICS_MAX_RADIUS == 127
    assert int(defines["PHNET_MASK_METRICS_MAX_SIZE"]) == hip_ops.MASK_METRICS_MAX_SIZE == hip_ops.LANE_DRAW_MAX_SIZE == 4096
    assert hip_ops.MASK_METRICS_COUNTS == V.COUNTS and len(V.COUNTS) == 7


def test_workspace_size(built):
    ws = built.phnet_mask_metrics_workspace
    assert ws(1, 1, 1, 0) == 16 and ws(1, 1, 64, 0) == 16 and ws(1, 1, 65, 0) == 32
    assert ws(3, 1080, 1920, 18) == 3 * 2 * 1080 * 30 * 8
    assert ws(0, 10, 10, 1) == 0
    assert ws(2, 4096, 4096, 127) == 2 * 2 * 4096 * 64 * 8
    for bad in ((-1, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4097, 4, 1), (1, 4, 4097, 1), (1, 4, 4, -1), (1, 4, 4, 128)):
        assert ws(*bad) == 0, bad


def test_validates_without_a_gpu(built):
    """Each refusal comes before any GPU call (this runs without a device).  Non-null pointers are made-up addresses - a call that
    got past the checks would try to launch."""
    p = 0x1000

    def run(pred=p, gt=p, n=2, h=40, w=70, radius=5, ws=p, ws_bytes=None, counts=p):
        if ws_bytes is None:
            ws_bytes = n * 2 * h * ((w + 63) // 64) * 8 if n > 0 and h > 0 and w > 0 else 0
        return built.phnet_mask_metrics(pred, gt, n, h, w, radius, ws, ws_bytes, counts, None)

    for key in ("pred", "gt", "ws", "counts"):
        assert run(**{key: None}) == ERR_ARG, key
    assert run(radius=128) == ERR_ARG and run(radius=-1) == ERR_ARG
    for side in (0, 4097, -3):
        assert run(h=side) == ERR_ARG and run(w=side) == ERR_ARG, side
    assert run(n=-1) == ERR_ARG
    assert run(ws_bytes=2 * 2 * 40 * 2 * 8 - 1) == ERR_ARG                          # one byte short
    assert run(ws_bytes=0) == ERR_ARG
    assert run(ws=p + 4) == ERR_ARG and run(counts=p + 4) == ERR_ARG                # 64-bit words
    assert run(n=1 << 21, h=4096, w=4096, radius=1, ws_bytes=1 << 62) == ERR_ARG    # more workgroups than a grid has
    # nothing to do: 0, whatever the pointers are; but the sizes are still checked
    assert run(n=0) == 0 and run(n=0, pred=None, gt=None, ws=None, counts=None, ws_bytes=0) == 0
    assert run(n=0, radius=128) == ERR_ARG and run(n=0, h=0) == ERR_ARG


def test_op_refuses_cpu_tensors_and_bad_shapes():
    from phnet_amd import hip_ops
    a = torch.zeros(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        hip_ops.mask_metric_counts(a, a, 2)
    with pytest.raises(RuntimeError, match="CUDA"):
        V.device_counts(a, a)
    with pytest.raises(RuntimeError, match="CUDA"):
        V.VideoMaskEval().update("v", a, a)


def test_kernels_compile_without_scratch_or_spills(tmp_path):
    """The compiler's resource metadata for csrc/mask_metrics.hip: no scratch, no spilled registers (the five-word window of the
    horizontal dilation must live in registers), and the tile of pass two within the 64 KB of LDS a launch gets unasked."""
    src = os.path.join(hip_build.CSRC, "mask_metrics.hip")
    out = subprocess.run([hip_build._hipcc(), *hip_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", str(tmp_path / "mask_metrics.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    assert len(names) == 2 and any("mask_boundary_kernel" in n for n in names) and any("mask_match_kernel" in n for n in names), names
    for key in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        vals = [int(v) for v in re.findall(key + r": (\d+)", out.stderr)]
        assert len(vals) == 2 and not any(vals), (key, vals)
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", out.stderr)]
    assert len(lds) == 2 and max(lds) <= 65536, lds
    print("VGPRs:", dict(zip(names, re.findall(r" VGPRs: (\d+)", out.stderr))), "LDS:", lds)


# ------------------------------------------------------------------------------------------------------------ the reference's values
def test_fixture_pins_what_it_is_meant_to():
    cases = C.fixture_cases()
    partial, branches, far = 0, set(), False
    for c in cases:
        n_fg, n_gt = int(c["bmap_pred"].sum()), int(c["bmap_gt"].sum())
        if n_fg and n_gt:
            k = C.counts(c["pred"], c["gt"], c["radius"])
            partial += 0.1 < c["F"] < 0.9 and 0 < k[5] < k[3] and 0 < k[6] < k[4]
            far |= c["F"] == 0
        else:
            branches.add((n_fg > 0, n_gt > 0))
    assert partial >= 3 and far and branches == {(False, True), (True, False), (False, False)}
    assert any(c["pred"].all() and not c["bmap_pred"].any() for c in cases)         # all foreground: an empty boundary map
    assert {c["radius"] for c in cases} >= {0, 1, 2, 3, 4, 5, 9}


@pytest.mark.parametrize("case", C.fixture_cases(), ids=lambda c: c["name"])
def test_restatement_reproduces_the_reference(case):
    pred, gt = case["pred"], case["gt"]
    assert np.array_equal(C.boundary_map(pred), case["bmap_pred"]) and np.array_equal(C.boundary_map(gt), case["bmap_gt"])
    assert V.boundary_radius(*pred.shape, case["bound_th"]) == case["radius"]
    k = C.counts(pred, gt, case["radius"])
    assert k.dtype == np.int64 and k.shape == (7,)
    assert float(V.boundary_f(k)) == case["F"]
    assert float(V.jaccard(k, pred.shape, two_class=False)) == case["J"]
    assert float(V.jaccard(k, pred.shape, two_class=True)) == case["J2"]
    # foreground is "not 0": any label value gives the same counts
    assert np.array_equal(C.counts(pred.astype(np.uint8) * 255, gt.astype(np.uint8) * 128, case["radius"]), k)


@pytest.mark.parametrize("h,w,radius", [(30, 90, 0), (30, 90, 1), (30, 90, 2), (40, 200, 18), (20, 90, 31), (16, 80, 65)])
def test_both_dilations_of_the_restatement_agree(h, w, radius):
    """`dilate` (nearest set pixel within the radius) is `dilate_scipy` (binary_dilation with the disk, what the fixture pins):
    on sparse points, where every pixel of the disk's outline shows, and on blobs."""
    rng = np.random.default_rng(radius)
    points = rng.random((h, w)) < 0.004
    points[0, 0] = points[-1, -1] = True
    for b in (points, C.boundary_map(C.blobs(h, w, radius)), np.zeros((h, w), bool)):
        assert np.array_equal(C.dilate(b, radius), C.dilate_scipy(b, radius))
    for c in C.fixture_cases():
        assert np.array_equal(C.dilate(c["bmap_gt"], c["radius"]), C.dilate_scipy(c["bmap_gt"], c["radius"]))


def test_restatement_takes_leading_dimensions():
    cases = [c for c in C.fixture_cases() if c["pred"].shape == (48, 80) and c["radius"] == 3]
    assert len(cases) >= 4
    pred, gt = np.stack([c["pred"] for c in cases[:4]]).reshape(2, 2, 48, 80), np.stack([c["gt"] for c in cases[:4]]).reshape(2, 2, 48, 80)
    k = C.counts(pred, gt, 3)
    assert k.shape == (2, 2, 7)
    for i, c in enumerate(cases[:4]):
        assert np.array_equal(k.reshape(4, 7)[i], C.counts(c["pred"], c["gt"], 3))
    assert np.array_equal(V.boundary_f(k).reshape(-1), [c["F"] for c in cases[:4]])


# ------------------------------------------------------------------------------------------------------------ host arithmetic
def test_boundary_radius():
    assert V.boundary_radius(96, 160) == 2 and V.boundary_radius(1080, 1920) == 18 and V.boundary_radius(4096, 4096) == 47
    assert V.boundary_radius(96, 160, 7) == 7 and V.boundary_radius(96, 160, 7.0) == 7 and V.boundary_radius(96, 160, 1) == 1
    assert V.boundary_radius(96, 160, 0) == 0 and V.boundary_radius(1, 1, 0.5) == 1
    for bad in (2.5, 1.000001, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            V.boundary_radius(96, 160, bad)


def test_f_branches_on_hand_made_counts():
    #                  areas      n_fg n_gt fgm gtm
    rows = np.array([[5, 5, 1, 0, 9, 0, 0],          # no predicted boundary: precision 1, recall 0
                     [5, 5, 1, 9, 0, 0, 0],          # no annotated boundary: precision 0, recall 1
                     [5, 0, 0, 0, 0, 0, 0],          # neither: 1
                     [5, 5, 1, 8, 4, 0, 0],          # both, nothing matched: precision + recall == 0 -> 0
                     [5, 5, 1, 8, 4, 2, 4],          # precision 1/4, recall 1
                     [5, 5, 1, 3, 7, 1, 3]], np.int64)
    f = V.boundary_f(rows)
    assert f.dtype == np.float64 and f.tolist() == [0.0, 0.0, 1.0, 0.0, 2 * 0.25 * 1.0 / 1.25, 2 * (1 / 3.0) * (3 / 7.0) / (1 / 3.0 + 3 / 7.0)]
    assert V.boundary_f(torch.from_numpy(rows)).tolist() == f.tolist()
    with pytest.raises(ValueError):
        V.boundary_f(rows.astype(np.float64))
    with pytest.raises(ValueError):
        V.boundary_f(rows[:, :6])


def test_jaccard_on_hand_made_counts():
    rows = np.array([[0, 0, 0, 0, 0, 0, 0], [6, 4, 2, 0, 0, 0, 0], [10, 0, 0, 0, 0, 0, 0]], np.int64)
    assert V.jaccard(rows, (4, 5), two_class=False).tolist() == [1.0, 2 / 8.0, 0.0]
    assert V.jaccard(rows, (4, 5), two_class=True).tolist() == [1.0, (2 + 12) / (8 + 18.0), (0 + 10) / (10 + 20.0)]
    # a 4096 x 4096 picture: the exact quotient, where a float32 denominator is not
    big = np.array([[3, 5, 1, 0, 0, 0, 0]], np.int64)
    assert float(V.jaccard(big, (4096, 4096))[0]) == (1 + (4096 * 4096 - 7)) / float(7 + (4096 * 4096 - 1))


def test_window_arithmetic():
    assert V.window_mean([1.0, 2.0, 6.0], None) == 3.0 and V.window_mean([1.0, 2.0, 6.0], 2) == 4.0 and V.window_mean([1.0, 2.0, 6.0], 480) == 3.0
    assert np.isnan(V.window_mean([], 480))

    def frames(f_values):                             # F = 1, J = 1 (no boundaries, equal masks) or F = 0, J = 1 / 3 (no predicted boundary)
        return np.array([[2, 2, 1 + (v > 0), 0, 0 if v else 3, 0, 0] for v in f_values], np.int64)

    ev = V.VideoMaskEval(window=3, two_class=False)
    ev.update_counts("a", frames([1, 1, 1]), (4, 4))
    ev.update_counts("a", frames([0, 0]), (4, 4))                                   # a second batch of the same video
    ev.update_counts("b", frames([1, 0, 0, 0]), (4, 4))
    ev.update_counts("c", frames([1]), (4, 4))
    ev.update_counts("d", frames([1, 1]), (4, 4))
    s = ev.summary()
    assert list(s["per_video"]) == ["a", "b", "c", "d"]
    assert [v["frames"] for v in s["per_video"].values()] == [5, 4, 1, 2]
    assert [v["F"] for v in s["per_video"].values()] == [1 / 3.0, 0.0, 1.0, 1.0]     # the LAST three frames of each video
    assert s["F"] == (0.0 + 1.0 + 1.0) / 3                                          # and the last three videos
    j, f = ev.frame_values("a")
    assert f.tolist() == [1.0, 1.0, 1.0, 0.0, 0.0] and j.tolist() == [1.0, 1.0, 1.0, 1 / 3.0, 1 / 3.0]
    plain = V.VideoMaskEval(window=None, two_class=False)
    for name in "abcd":
        for counts, hw in ev._videos[name]:
            plain.update_counts(name, counts, hw)
    p = plain.summary()
    assert [v["F"] for v in p["per_video"].values()] == [3 / 5.0, 1 / 4.0, 1.0, 1.0] and p["F"] == (0.6 + 0.25 + 1.0 + 1.0) / 4
    assert V.VideoMaskEval().window == 480 and V.VideoMaskEval().two_class
    with pytest.raises(ValueError):
        V.VideoMaskEval(window=0)
    block = V.result_block(s, "lists/val.txt")
    assert "Results (val.txt)" in block and "a: J" in block and "\nF: 0.6667\n" in block


def test_command_line_without_arguments_prints_usage(capsys):
    assert V.main([]) == 2 and V.main(["-h"]) == 0
    assert "python -m phnet_amd.evaluation.video" in capsys.readouterr().out
    assert V.main(["-a", "x", "-d", "y", "-l", "/nonexistent/list", "-r", "4", "-c", "4", "-w", "3"]) == 1
