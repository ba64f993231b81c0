"""Host side of the temporal stability evaluator (phnet_amd/evaluation/temporal.py), no GPU: with a numpy stand-in for its one
device step the module reproduces the counts the reference's executed evalTemporalOLV2.py gave on the fixture, the counting
rules hold on hand-made matrices, and `phnet_lane_iou_groups` / its wrapper refuse bad arguments before any launch or upload."""
import ctypes

import numpy as np
import pytest
import torch

from phnet_amd import _lib
from phnet_amd.evaluation import temporal as T
from tests import temporal_cases as C


@pytest.fixture(scope="module")
def built():
    from phnet_amd import build
    return build.build(verbose=False)


@pytest.fixture(scope="module")
def fx():
    return C.fixture()


# ---------------------------------------------------------------------------------------------- the reference's counts
@pytest.mark.parametrize("thr", [0.5, 0.8])
def test_host_logic_reproduces_the_reference_counts(fx, thr, tmp_path):
    want = fx["expected"][repr(thr)]
    per_video = {v: T.evaluate_frames(C.frames_of(fx, v, T), fx["height"], fx["width"], fx["lane_width"], thr, ious=C.numpy_ious)
                 for v in fx["videos"]}
    C.check_against_fixture(T.summarize(per_video), want)
    assert [sum(t[i] for t in per_video[v]) for v in per_video for i in range(3)] == \
           [n for v in per_video for n in want["video_totals"][v]]
    # the same through the files, in other batch sizes (the carried frame is drawn again: nothing may change)
    anno_dir, pred_dir, names = C.write_files(fx, str(tmp_path))
    for batch in (1, 3):
        res = T.evaluate(anno_dir, pred_dir, names, fx["height"], fx["width"], fx["lane_width"], thr, batch_frames=batch,
                         ious=C.numpy_ious)
        C.check_against_fixture(res, want)


def test_fixture_is_not_degenerate(fx):
    want = fx["expected"]["0.5"]
    assert min(want["Ns"], want["Nj"], want["Nm"]) >= 2
    assert sorted(len(f) for f in fx["videos"].values()) == [1, 8, 10, 12]
    assert any(f["pred"] == "" for v in fx["videos"].values() for f in v) and any(f["anno"] == "" for v in fx["videos"].values() for f in v)
    assert fx["expected"]["0.8"]["Nm"] > want["Nm"]                      # the stricter threshold loses detections


# ---------------------------------------------------------------------------------------------- counting rules on hand-made matrices
def _res(rows):
    return T.match_results(np.asarray(rows, np.float64))


def test_equality_at_the_threshold_counts_as_stable():
    M = np.array([[0.9]])
    assert T.count_inter_frame(M, _res([[0.5]]), _res([[0.5]]), 0.5) == (1, 0, 0)
    assert T.count_inter_frame(M, _res([[0.5]]), _res([[0.9]]), 0.5) == (1, 0, 0)     # neither > nor <: falls through, as there
    assert T.count_inter_frame(M, _res([[0.5]]), _res([[0.1]]), 0.5) == (1, 0, 0)
    assert T.count_inter_frame(M, _res([[0.6]]), _res([[0.1]]), 0.5) == (0, 1, 0)
    assert T.count_inter_frame(M, _res([[0.1]]), _res([[0.6]]), 0.5) == (0, 1, 0)
    assert T.count_inter_frame(M, _res([[0.4]]), _res([[0.1]]), 0.5) == (0, 0, 1)
    assert T.count_inter_frame(M, _res([[0.6]]), _res([[0.7]]), 0.5) == (1, 0, 0)
    assert T.count_inter_frame(np.array([[0.5]]), _res([[0.9]]), _res([[0.9]]), 0.5) == (0, 0, 0)   # M itself wants IoU > threshold


def test_annotated_lane_without_a_partner_is_not_counted():
    # two lanes now, one before: the assignment gives the old lane to the better of them, the other one is new
    M = np.array([[0.7], [0.9]])
    R_t, R_prev = _res([[0.1, 0.9], [0.1, 0.2]]), _res([[0.9]])
    assert T.persistent_lanes(M, 0.5)[0].tolist() == [1]
    assert T.count_inter_frame(M, R_t, R_prev, 0.5) == (0, 1, 0)         # lane 1 gets prediction 0 (0.1) now, had 0.9 before
    # a pair below the threshold is no persistent lane
    assert T.count_inter_frame(np.array([[0.3]]), _res([[0.9]]), _res([[0.9]]), 0.5) == (0, 0, 0)
    # no annotation on one side: nothing persists
    assert T.count_inter_frame(np.zeros((0, 2)), _res(np.zeros((0, 3))), _res([[0.9], [0.8]]), 0.5) == (0, 0, 0)
    assert T.count_inter_frame(np.zeros((2, 0)), _res([[0.9], [0.8]]), _res(np.zeros((0, 3))), 0.5) == (0, 0, 0)


def test_frame_without_predictions_gives_zero_iou_on_that_side():
    M = np.array([[0.9]])
    empty = T.match_results(np.zeros((1, 0)))
    assert T.count_inter_frame(M, empty, _res([[0.9]]), 0.5) == (0, 1, 0)
    assert T.count_inter_frame(M, _res([[0.9]]), empty, 0.5) == (0, 1, 0)
    assert T.count_inter_frame(M, empty, empty, 0.5) == (0, 0, 1)
    # more annotated lanes than predictions: the one left over has IoU 0
    R = _res([[0.9], [0.8]])
    assert T.count_inter_frame(np.array([[0.9, 0.0], [0.0, 0.9]]), R, R, 0.5) == (1, 0, 1)


def test_videos_rates_and_num_t(fx):
    one = C.frames_of(fx, "seq_d", T)
    assert len(one) == 1 and T.evaluate_frames(one, 96, 160, 12, ious=C.numpy_ious) == []
    assert T.evaluate_frames([], 96, 160, 12, ious=C.numpy_ious) == []
    res = T.summarize({"v": []})
    assert (res["Ns"], res["Nj"], res["Nm"]) == (0, 0, 0) and all(np.isnan(res[k]) for k in ("Rs", "Rj", "Rm"))
    res = T.summarize({"a": [(1, 0, 0), (2, 1, 0)], "b": [(0, 0, 4)]})
    assert (res["Ns"], res["Nj"], res["Nm"], res["Rs"], res["Rj"], res["Rm"]) == (3, 1, 4, 3 / 8, 1 / 8, 4 / 8)
    with pytest.raises(ValueError):
        T.evaluate_frames(one, 96, 160, 12, num_t=2, ious=C.numpy_ious)
    with pytest.raises(ValueError):
        T.evaluate("a", "b", ["v/0"], 96, 160, num_t=2, ious=C.numpy_ious)
    assert T.video_datalist(["b/1", "a/1", "b/2", "c/x/1"]) == {"b": ["b/1", "b/2"], "a": ["a/1"], "c/x": ["c/x/1"]}
    block = T.result_block({"Ns": 3, "Nj": 1, "Nm": 4, "Rs": 0.375, "Rj": 0.125, "Rm": 0.5}, "/x/list.txt")
    assert block == ("====================Results (list.txt)====================\nNs: 3\nNj: 1\nNm: 4\nRs: 0.3750\nRj: 0.1250\n"
                     "Rm: 0.5000\n" + "=" * 58 + "\n")


def test_files_spline_and_segments(tmp_path):
    p = tmp_path / "f.lines.txt"
    p.write_text("1 2 3 4 5.5 6\n7 8\n\n10.25 20 30 40 \n")
    assert T.load_lanes(str(p)) == [[(1.0, 2.0), (3.0, 4.0), (5.5, 6.0)], [(10.25, 20.0), (30.0, 40.0)]]     # the one-point lane is dropped
    assert T.load_lanes(str(tmp_path / "missing.lines.txt")) == []
    assert T.lanes_from_text("") == []
    with pytest.raises(ValueError):
        T.lanes_from_text("1 2 3\n")
    # truncation toward zero, not rounding; clamped to the raster kernel's range
    assert T.lane_segments(np.array([[-0.7, 3.9], [5.5, -2.9], [1e6, -1e6]])).tolist() == [[0, 3, 5, -2], [5, -2, 8192, -8192]]
    assert T.lane_segments(np.zeros((1, 2))).shape == (0, 4)
    seg = T.lane_segments(T.lane_polyline([(3.0, 80.0), (9.0, 50.0), (11.0, 20.0)]))
    assert seg.shape == (10, 4) and seg.dtype == np.int32 and seg.flags.c_contiguous       # rows of (x0, y0, x1, y1) for the device
    # the spline passes through its points, (len - 1) * 5 + 1 of them; degree min(3, len - 1)
    for n in (2, 3, 4, 7):
        pts = [(10.0 + 3 * i + (i % 2), 90.0 - 11 * i) for i in range(n)]
        poly = T.interp(pts, n=5)
        assert poly.shape == ((n - 1) * 5 + 1, 2)
        assert np.allclose(poly[0], pts[0]) and np.allclose(poly[-1], pts[-1])
    two = T.interp([(0.0, 0.0), (10.0, 20.0)], n=5)
    assert np.allclose(two, np.linspace(0, 1, 6)[:, None] * np.array([10.0, 20.0]))
    # duplicates are removed in order before the spline; fewer than two distinct points: no pixels
    assert np.array_equal(T.lane_polyline([(1, 2), (1, 2), (5, 9), (1, 2)]), T.interp([(1.0, 2.0), (5.0, 9.0)], n=5))
    assert T.lane_polyline([(4, 4), (4, 4)]).shape == (0, 2)


def test_frame_ious_layout_and_single_drawing():
    calls = []

    def backend(segments, groups, h, w, lw):
        calls.append((len(segments), np.asarray(groups).tolist()))
        return C.numpy_ious(segments, groups, h, w, lw)

    a0 = [[(10.0, 50.0), (12.0, 5.0)], [(40.0, 50.0), (42.0, 5.0)]]
    a1 = [[(11.0, 50.0), (13.0, 5.0)]]
    p1 = [[(11.0, 50.0), (13.0, 5.0)], [(70.0, 50.0), (70.0, 5.0)], [(41.0, 50.0), (41.0, 5.0)]]
    R, M = T.frame_ious([(a0, []), (a1, p1), ([], p1)], None, 60, 90, 8, backend)
    assert calls == [(2 + 0 + 1 + 3 + 0 + 3, [[0, 2, 2, 0, 0], [2, 1, 3, 3, 0], [2, 1, 0, 2, 3], [6, 0, 6, 3, 5], [6, 0, 2, 1, 5]])]
    assert [r.shape for r in R] == [(2, 0), (1, 3), (0, 3)] and M[0] is None and [m.shape for m in M[1:]] == [(1, 2), (0, 1)]
    assert 1.0 - 1e-12 < R[1][0, 0] < 1.0 and R[1][0, 1] == 0.0 and 0.6 < M[1][0, 0] < 0.9 and M[1][0, 1] == 0.0     # eps keeps IoU below 1
    # with the previous frame carried in, the first frame gets its M too
    R2, M2 = T.frame_ious([(a1, p1)], a0, 60, 90, 8, backend)
    assert np.array_equal(R2[0], R[1]) and np.array_equal(M2[0], M[1])


# ---------------------------------------------------------------------------------------------- the C ABI and its wrapper
def test_iou_groups_argument_validation_needs_no_gpu(built):
    lib = _lib.lib()
    f = lib.phnet_lane_iou_groups
    assert dict((n, a) for n, _, a in _lib.declared_functions())["phnet_lane_iou_groups"][8] is ctypes.c_double
    # (masks, n_lanes, height, width, groups, n_groups, n_entries, scale, eps, iou, area, stream)
    assert f(None, 2, 64, 96, None, 1, 4, 1, 0.0, None, None, None) == -1          # null outputs where work exists
    assert f(None, 2, 64, 96, None, 0, 0, 1, 0.0, None, None, None) == 0           # no groups: no-op
    assert f(None, 2, 64, 96, None, 3, 0, 1, 0.0, None, None, None) == 0           # no entries: no-op
    assert f(None, 2, 5000, 96, None, 0, 0, 1, 0.0, None, None, None) == -1
    assert f(None, 2, 64, 0, None, 0, 0, 1, 0.0, None, None, None) == -1
    assert f(None, 2, 64, 96, None, 0, 0, 0, 0.0, None, None, None) == -1          # scale
    for eps in (-1.0, float("nan"), float("inf")):
        assert f(None, 2, 64, 96, None, 0, 0, 3, eps, None, None, None) == -1
    assert f(None, -1, 64, 96, None, 0, 0, 1, 0.0, None, None, None) == -1
    assert f(None, 2, 64, 96, None, -1, 0, 1, 0.0, None, None, None) == -1
    assert f(None, 2, 64, 96, None, 1, -1, 1, 0.0, None, None, None) == -1


def test_wrapper_checks_the_group_table_before_any_upload():
    from phnet_amd import hip_ops as K
    masks = torch.zeros((4, 8, 1), dtype=torch.int32)                     # a host tensor: reaching the upload would raise RuntimeError
    good = [[0, 2, 2, 2, 0], [0, 0, 0, 2, 4], [3, 1, 3, 1, 4]]
    table, n = K.check_iou_groups(good, 4)
    assert n == 5 and table.dtype == np.int32 and table.tolist() == good
    assert K.check_iou_groups(np.zeros((0, 5), np.int32), 0)[1] == 0
    for bad in ([[0, 2, 2, 2, 0], [3, 1, 3, 1, 5]],                       # a gap in out_first
                [[0, 2, 2, 2, 1]],                                        # does not start at 0
                [[0, 2, 2, 2, 0], [0, 1, 0, 1, 3]],                       # overlaps
                [[0, 2, 3, 2, 0]],                                        # columns 3, 4 of 4 lanes
                [[-1, 1, 0, 1, 0]],
                [[0, -1, 0, 1, 0]],
                [[0, 1, 0, 1]]):
        with pytest.raises(ValueError):
            K.lane_iou_groups(masks, bad, 20)
    with pytest.raises(ValueError):
        K.lane_iou_groups(masks, good, 20, scale=0)
    with pytest.raises(ValueError):
        K.lane_iou_groups(masks, good, 20, eps=float("nan"))
    with pytest.raises(RuntimeError):
        K.lane_iou_groups(masks, good, 20)                                # a good table gets as far as the device check
