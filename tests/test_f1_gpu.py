"""Validation F1 on the device (csrc/lane_eval.hip, phnet_amd/evaluation/online.py): the two kernels against the numpy restatement
of tests/f1_cases.py bit for bit (which tests/test_f1_cpu.py holds to the host evaluator), the meter against `culane.evaluate` on
the files the writer produces, batching, per-video rows, reset, graph capture and one case at the full geometry."""
import functools

import numpy as np
import pytest
import torch

from tests import f1_cases as C

pytestmark = pytest.mark.gpu
POISON = 0x5a5a5a5a
TABLE_NAMES = [name for name, _, _ in C.table_cases()]


@pytest.fixture(scope="module")
def ops():
    from phnet_amd import hip_ops
    return hip_ops


@functools.lru_cache(maxsize=None)
def _case(name):
    """(mode, tables, restated segs, restated lane_pts) - computed once, shared, never written."""
    mode, t = {n: (m, t) for n, m, t in C.table_cases()}[name]
    segs, lane_pts = C.segment_table(t, mode)
    return mode, t, segs, lane_pts


def _cuda(t):
    return {k: torch.from_numpy(v).cuda() for k, v in t.items()}


def _meter(mode="wire", max_images=6, videos=1, **kw):
    from phnet_amd.evaluation.online import LaneF1Meter
    opt = dict(height=C.H, width=C.W, lane_width=C.LANE_W, threshold=C.THRESHOLD, size=C.SIZE, crop_top=C.CROP_TOP,
               max_images=max_images, max_gt_lanes=C.G, max_gt_points=C.P, max_lanes=C.L, n_offsets=C.S, videos=videos, mode=mode)
    opt.update(kw)
    return LaneF1Meter(**opt)


def _update(meter, d, sel=None, video=None):
    pick = (lambda x: x) if sel is None else (lambda x: x[sel].contiguous())
    meter.update(dict(points=pick(d["points"]), count=pick(d["count"]), lanes_num=pick(d["lanes_num"])),
                 pick(d["gt_points"]), pick(d["gt_count"]), pick(d["gt_num"]), video=video)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


# ------------------------------------------------------------------------------------------------ kernels against the restatement
@pytest.mark.parametrize("name", TABLE_NAMES)
def test_segment_table_bit_exact(ops, name):
    mode, t, want_segs, want_pts = _case(name)
    d = _cuda(t)
    f = t["gt_num"].shape[0]
    out = dict(segs=torch.full((f * (C.G + C.L), C.C, 5), POISON, dtype=torch.int32, device="cuda"),
               lane_pts=torch.full((f, C.G + C.L), POISON, dtype=torch.int32, device="cuda"))
    got = ops.lane_eval_segments(d["points"], d["count"], d["lanes_num"], d["gt_points"], d["gt_count"], d["gt_num"], mode, C.SIZE,
                                 C.CROP_TOP, out=out)
    segs, lane_pts = got["segs"].cpu().numpy(), got["lane_pts"].cpu().numpy()
    assert np.array_equal(lane_pts, want_pts)
    bad = np.argwhere(segs != want_segs)
    assert len(bad) == 0, (name, bad[:5], segs[tuple(bad[0][:2])] if len(bad) else None, want_segs[tuple(bad[0][:2])] if len(bad) else None)
    fresh = ops.lane_eval_segments(d["points"], d["count"], d["lanes_num"], d["gt_points"], d["gt_count"], d["gt_num"], mode, C.SIZE, C.CROP_TOP)
    assert np.array_equal(fresh["segs"].cpu().numpy(), want_segs)


@pytest.mark.parametrize("name", [n for n, _, _ in C.matrix_cases()])
def test_matching_and_counters_bit_exact(ops, name):
    iou, lane_pts = {n: (m, p) for n, m, p in C.matrix_cases()}[name]
    f, g, l = iou.shape
    video = np.array([0, 2, 1, 1, 5, 0], np.int32)                                  # row 5 does not exist: in no total
    start_tot = np.arange(12, dtype=np.int64).reshape(3, 4) * 7
    start_iou = np.array([0.1, 2.5, 1.0 / 3.0])
    for vid, tot0, iou0 in ((None, start_tot[:1], start_iou[:1]), (video, start_tot, start_iou)):
        want = C.count_images(iou, lane_pts, C.THRESHOLD, vid, tot0, iou0)
        totals, iou_tot = torch.from_numpy(tot0.copy()).cuda(), torch.from_numpy(iou0.copy()).cuda()
        overflow = torch.full((1,), 3, dtype=torch.int32, device="cuda")
        out = dict(tp=torch.full((f,), POISON, dtype=torch.int32, device="cuda"), fp=torch.full((f,), POISON, dtype=torch.int32, device="cuda"),
                   fn=torch.full((f,), POISON, dtype=torch.int32, device="cuda"),
                   iou_im=torch.full((f,), -7.0, dtype=torch.float64, device="cuda"),
                   anno_match=torch.full((f, g), POISON, dtype=torch.int32, device="cuda"))
        got = ops.lane_eval_count(torch.from_numpy(iou).cuda(), torch.from_numpy(lane_pts).cuda(), g, C.THRESHOLD, totals, iou_tot, overflow,
                                  video=None if vid is None else torch.from_numpy(vid).cuda(), out=out)
        for k in ("tp", "fp", "fn", "anno_match"):
            assert np.array_equal(got[k].cpu().numpy(), want[k]), (name, k, got[k].cpu().numpy(), want[k])
        assert _same_bits(got["iou_im"].cpu().numpy(), want["iou_im"]), (got["iou_im"].cpu().numpy(), want["iou_im"])
        assert np.array_equal(totals.cpu().numpy(), want["totals"])
        assert _same_bits(iou_tot.cpu().numpy(), want["iou_tot"])
        assert int(overflow.cpu()[0]) == 3 and want["overflow"] == 0                 # added to, and nothing to add


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_meter_rows_equal_the_restatement_on_the_device_iou(name):
    """The whole chain per case: the IoU matrices come from the existing mask kernels on the segment table; the rows of the count
    kernel must be what the count rules give on exactly those matrices."""
    mode, t, _, want_pts = _case(name)
    f = t["gt_num"].shape[0]
    meter = _meter(mode)
    _update(meter, _cuda(t))
    rows = meter.per_image()
    assert np.array_equal(rows["lane_pts"], want_pts)
    iou = rows["iou"]
    want = C.count_images(iou, want_pts, C.THRESHOLD)
    for k in ("tp", "fp", "fn", "anno_match"):
        assert np.array_equal(rows[k], want[k]), (name, k)
    assert _same_bits(rows["iou_im"], want["iou_im"])
    res = meter.compute()
    assert (res["tp"], res["fp"], res["fn"], res["images"], res["overflow"]) == (*want["totals"][0, :3].tolist(), f, 0)
    assert _same_bits([res["miou"]], [want["iou_tot"][0] / f]) or (res["miou"] != res["miou"] and want["iou_tot"][0] != want["iou_tot"][0])
    if name in ("edge", "raw-edge"):
        assert np.isnan(iou[2, 0, 0]) and rows["tp"][2] == 0                          # two empty masks: NaN IoU, no match
        assert want_pts[2, 1] == 1 and rows["anno_match"][2, 1] == -1                 # the 1-point lane: sim 0, not NaN


# ------------------------------------------------------------------------------------------------ end to end against the files
class _Lane:
    def __init__(self, points):
        self.points = points


def _fmt(v):
    return repr(float(v))                                                              # round-trips a float32 (and nan / inf)


def _write_files(tmp_path, cases, size, g, l, s, p):
    """The predictions through the writer, the annotations as text -> (anno_dir, detect_dir, names)."""
    from phnet_amd.evaluation import generate_lane
    names = []
    (tmp_path / "anno" / "v").mkdir(parents=True, exist_ok=True)
    for ci, t in enumerate(cases):
        for f in range(t["gt_num"].shape[0]):
            stem = f"{ci}_{f:02d}"
            n = min(max(int(t["lanes_num"][f]), 0), l)
            lanes = [_Lane(t["points"][f, k, :min(max(int(t["count"][f, k]), 0), s)].astype(np.float64)) for k in range(n)]
            generate_lane.generate_predV2(dict(name="v", ImgName=[stem], size=size), lanes, 0, str(tmp_path / "det"))
            n = min(max(int(t["gt_num"][f]), 0), g)
            anno = [t["gt_points"][f, j, :min(max(int(t["gt_count"][f, j]), 0), p)] for j in range(n)]
            (tmp_path / "anno" / "v" / (stem + ".lines.txt")).write_text(
                "".join(" ".join(f"{_fmt(x)} {_fmt(y)}" for x, y in lane) + "\n" for lane in anno))
            names.append(f"/v/{stem}.jpg")
    return str(tmp_path / "anno"), str(tmp_path / "det"), names


def test_meter_equals_the_file_evaluator(tmp_path, monkeypatch):
    from phnet_amd.evaluation import culane, generate_lane
    monkeypatch.setattr(generate_lane, "CROP_TOP", C.CROP_TOP)                         # the writer's constant, at the cases' crop
    cases = [t for _, mode, t in C.table_cases() if mode == "wire"]
    a_dir, d_dir, names = _write_files(tmp_path, cases, C.SIZE, C.G, C.L, C.S, C.P)
    want = culane.evaluate(a_dir, d_dir, names, C.W, C.H, C.LANE_W, C.THRESHOLD, str(tmp_path / "out.txt"), batch_images=4)
    want_text = (tmp_path / "out.txt").read_text()
    assert want["tp"] > 0 and want["fp"] > 0 and want["fn"] > 0 and 0 < want["miou"] < 1                # not degenerate
    meter = _meter("wire")
    for t in cases:
        _update(meter, _cuda(t))
    got = meter.compute()
    assert (got["tp"], got["fp"], got["fn"], got["images"]) == (want["tp"], want["fp"], want["fn"], len(names))
    assert _same_bits([got["miou"]], [want["miou"]])
    for k in ("precision", "recall", "Fmeasure"):
        assert got[k] == want[k]
    dev = culane.evaluate(a_dir, d_dir, names, C.W, C.H, C.LANE_W, C.THRESHOLD, str(tmp_path / "out.txt"), batch_images=4, device_pipeline=True)
    assert set(dev) == set(want)
    for k in want:
        assert dev[k] == want[k] or (dev[k] != dev[k] and want[k] != want[k]), (k, dev[k], want[k])
    assert (tmp_path / "out.txt").read_text() == want_text
    empty = culane.evaluate(a_dir, d_dir, [], C.W, C.H, C.LANE_W, C.THRESHOLD, device_pipeline=True)
    assert empty["tp"] == 0 and empty["miou"] != empty["miou"]


def test_full_geometry(tmp_path, ops):
    from phnet_amd.evaluation import culane
    t, opt = C.full_geometry_case()
    g, l, s, p = t["gt_count"].shape[1], t["count"].shape[1], t["points"].shape[2], t["gt_points"].shape[2]
    want_segs, want_pts = C.segment_table(t, "wire", opt["size"], opt["crop_top"])
    d = _cuda(t)
    got = ops.lane_eval_segments(d["points"], d["count"], d["lanes_num"], d["gt_points"], d["gt_count"], d["gt_num"], "wire", opt["size"],
                                 opt["crop_top"])
    assert np.array_equal(got["lane_pts"].cpu().numpy(), want_pts) and np.array_equal(got["segs"].cpu().numpy(), want_segs)
    meter = _meter("wire", max_images=2, max_gt_lanes=g, max_gt_points=p, max_lanes=l, n_offsets=s,
                   **{k: opt[k] for k in ("height", "width", "lane_width", "threshold", "size", "crop_top")})
    _update(meter, d)
    rows, res = meter.per_image(), meter.compute()
    want = C.count_images(rows["iou"], want_pts, opt["threshold"])
    assert np.array_equal(rows["anno_match"], want["anno_match"]) and _same_bits(rows["iou_im"], want["iou_im"])
    a_dir, d_dir, names = _write_files(tmp_path, [t], opt["size"], g, l, s, p)         # the writer with its own crop_top = 480
    ref = culane.evaluate(a_dir, d_dir, names, opt["width"], opt["height"], opt["lane_width"], opt["threshold"])
    assert (res["tp"], res["fp"], res["fn"]) == (ref["tp"], ref["fp"], ref["fn"]) and res["tp"] >= 1
    assert _same_bits([res["miou"]], [ref["miou"]])


# ------------------------------------------------------------------------------------------------ batching, videos, reset, graphs
def test_batching_videos_and_reset():
    _, t, _, _ = _case("regular")
    d = _cuda(t)
    whole = _meter("wire")
    _update(whole, d)
    one = whole.compute()
    rows = whole.per_image()
    halves = _meter("wire", max_images=3)
    lo, hi = torch.arange(0, 3, device="cuda"), torch.arange(3, 6, device="cuda")
    _update(halves, d, lo)
    first = halves.per_image()
    _update(halves, d, hi)
    second = halves.per_image()
    two = halves.compute()
    for k in one:
        assert two[k] == one[k] or (two[k] != two[k] and one[k] != one[k]), k
    for k in rows:
        assert np.array_equal(np.concatenate([first[k], second[k]]), rows[k], equal_nan=k in ("iou_im", "iou")), k
    # per-video rows against one meter per video
    video = np.array([0, 1, 0, 1, 1, 0], np.int32)
    multi = _meter("wire", videos=2)
    _update(multi, d, video=torch.from_numpy(video).cuda())
    both = multi.compute()
    assert (both["tp"], both["fp"], both["fn"], both["images"]) == (one["tp"], one["fp"], one["fn"], 6)
    for v in range(2):
        single = _meter("wire")
        _update(single, d, torch.from_numpy(np.nonzero(video == v)[0]).cuda())
        want = single.compute()
        for k in ("tp", "fp", "fn", "precision", "recall", "Fmeasure"):
            assert both["per_video"][v][k] == want[k], (v, k)
        assert _same_bits([both["per_video"][v]["miou"]], [want["miou"]])
    assert set(both["aggregate"]) == {"miou", "F1", "p", "r"}
    # reset clears
    multi.reset()
    cleared = multi.compute()
    assert (cleared["tp"], cleared["fp"], cleared["fn"], cleared["images"], cleared["overflow"]) == (0, 0, 0, 0, 0)
    _update(whole, d)
    assert whole.compute()["images"] == 12                                             # accumulates until reset
    whole.reset()
    _update(whole, d)
    again = whole.compute()
    for k in one:
        assert again[k] == one[k] or (again[k] != again[k] and one[k] != one[k]), k


def test_update_in_a_captured_graph_equals_eager():
    """A linear single-stream graph; a host synchronisation or an allocation inside `update` would fail the capture."""
    _, t, _, _ = _case("regular")
    flipped = {k: v[::-1].copy() for k, v in t.items()}
    live = _cuda(t)
    meter = _meter("wire")
    _update(meter, live)                                                               # warm-up: every kernel is loaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _update(meter, live)
    for tables in (flipped, t):
        for k, v in tables.items():
            live[k].copy_(torch.from_numpy(v))
        meter.reset()
        graph.replay()
        torch.cuda.synchronize()
        got_rows, got = meter.per_image(), meter.compute()
        eager = _meter("wire")
        _update(eager, _cuda(tables))
        want_rows, want = eager.per_image(), eager.compute()
        assert got["images"] == 6
        for k in want:
            assert got[k] == want[k] or (got[k] != got[k] and want[k] != want[k]), k
        for k in want_rows:
            assert np.array_equal(got_rows[k], want_rows[k], equal_nan=k in ("iou_im", "iou")), k
    graph.replay(); graph.replay()
    torch.cuda.synchronize()
    assert meter.compute()["images"] == 18                                             # replays accumulate like updates
