"""Validation F1 on the device, the part that needs no GPU: the numpy restatement of the rules (tests/f1_cases.py) is held to the
host evaluator it restates - phnet_amd/evaluation/culane.py and generate_lane.py - on every shared case, so that a kernel equal to
the restatement (tests/test_f1_gpu.py) is equal to the file protocol; plus the library's exports and argument checks."""
import ctypes
import math

import numpy as np
import pytest

from phnet_amd import _lib
from phnet_amd.evaluation import culane, generate_lane
from tests import f1_cases as C


def _bits(a):
    """float32 bit patterns with every NaN folded into one (a NaN has no agreed payload on either side)."""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(a != a, np.uint32(0x7fc00000), a.view(np.uint32))


def _present_lanes():
    """Every present lane of every table case, in evaluator coordinates: (case, image, lane index, float32 [n,2])."""
    for name, mode, t in C.table_cases():
        f_, n = t["gt_num"].shape[0], t["gt_count"].shape[1] + t["count"].shape[1]
        for f in range(f_):
            for j in range(n):
                present, lane = C.lane_of(t, f, j, mode)
                if present:
                    yield name, f, j, lane


@pytest.fixture(scope="module")
def built():
    from phnet_amd import build
    return build.build(verbose=False)


def test_cases_cover_what_the_issue_lists():
    lanes = list(_present_lanes())
    sizes = {len(lane) for _, _, _, lane in lanes}
    assert {0, 1, 2, 3, 4, 5, C.P, C.S} <= sizes
    assert any(np.isinf(lane).any() for *_, lane in lanes) and any(np.isnan(lane).any() for *_, lane in lanes)
    assert any(len(lane) > 2 and (lane[1:] == lane[:-1]).all(axis=1).any() for *_, lane in lanes)          # a repeated point
    by_mode = {mode: t for name, mode, t in C.table_cases() if name in ("regular", "raw")}
    # a 2-point prediction: dropped by the wire filter, kept in raw mode
    assert (by_mode["wire"]["count"][0] == 2).any() and not C.lane_of(by_mode["wire"], 0, C.G + 2, "wire")[0]
    assert (by_mode["raw"]["count"][0] == 2).any() and C.lane_of(by_mode["raw"], 0, C.G + 2, "raw")[0]
    limits = dict((n, t) for n, _, t in C.table_cases())["limits"]
    assert limits["gt_num"].max() > C.G and limits["gt_count"].max() > C.P and limits["count"].max() > C.S and limits["lanes_num"].max() > C.L
    assert limits["gt_count"].min() < 0 and limits["count"].min() < 0 and limits["lanes_num"].min() < 0


def test_spline_points_equal_the_host_evaluator_bit_for_bit():
    """Also the condition of the rule: on these lanes the product-form cube and np.power agree in float32."""
    seen = 0
    lanes = [lane for *_, lane in _present_lanes()]
    t, _ = C.full_geometry_case()
    lanes += [C.lane_of(t, f, j, "wire", (800, 1920), 480)[1] for f in range(2) for j in range(8) if C.lane_of(t, f, j, "wire", (800, 1920), 480)[0]]
    for lane in lanes:
        if len(lane) < 3:
            continue
        want = culane.spline_interp_times(lane, 50)
        got = C.polyline(lane)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(_bits(got), _bits(want))
        seen += 1
    assert seen >= 30


def test_segments_equal_the_host_evaluator():
    for name, f, j, lane in _present_lanes():
        if len(lane) < 2:
            continue
        q = C.end_points(C.polyline(lane))
        assert np.array_equal(np.concatenate([q[:-1], q[1:]], axis=1), culane.lane_segments(lane)), (name, f, j)
    for name, mode, t in C.table_cases():
        segs, lane_pts = C.segment_table(t, mode)
        assert segs.shape == (t["gt_num"].shape[0] * (C.G + C.L), C.C, 5)
        for lane_id in range(segs.shape[0]):
            f, j = divmod(lane_id, C.G + C.L)
            present, lane = C.lane_of(t, f, j, mode)
            want = culane.lane_segments(lane) if present and len(lane) >= 2 else np.zeros((0, 4), np.int32)
            n = len(want)
            assert np.array_equal(segs[lane_id, :n, :4], want) and (segs[lane_id, :n, 4] == lane_id).all()
            assert (segs[lane_id, n:, 4] == -1).all() and not segs[lane_id, n:, :4].any()
            assert lane_pts[f, j] == (len(lane) if present else -1)


class _Lane:
    def __init__(self, points):
        self.points = points


def _through_the_file(tmp_path, lanes, size, crop_top):
    text = "".join("".join("%.1f %.1f " % (tx * size[1] / 2, (ty * size[0] + crop_top) / 2) for tx, ty in reversed(pts)) + "\n"
                   for pts in lanes if len(pts) > 2)
    path = tmp_path / "x.lines.txt"
    path.write_text(text)
    return culane.read_lane_file(str(path))


def test_wire_rule_equals_the_text_round_trip(tmp_path):
    # the writer itself, at its own crop_top, on the predictions of the full-geometry case
    t, opt = C.full_geometry_case()
    assert opt["crop_top"] == generate_lane.CROP_TOP
    for f in range(2):
        n = int(t["lanes_num"][f])
        lanes = [_Lane(t["points"][f, k, :t["count"][f, k]].astype(np.float64)) for k in range(n)]
        path = generate_lane.generate_predV2(dict(name="v", ImgName=["a"], size=opt["size"]), lanes, 0, str(tmp_path))
        back = culane.read_lane_file(path)
        mine = [C.lane_of(t, f, 4 + k, "wire", opt["size"], opt["crop_top"]) for k in range(n)]
        mine = [lane for present, lane in mine if present]
        assert len(back) == len(mine) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(back, mine))
    # the same format at the cases' crop_top (the writer's is a constant), on every wire case: NaN, +-inf, exact ties
    for name, mode, tab in C.table_cases():
        if mode != "wire":
            continue
        for f in range(tab["lanes_num"].shape[0]):
            n = min(max(int(tab["lanes_num"][f]), 0), C.L)
            raw = [tab["points"][f, k, :min(max(int(tab["count"][f, k]), 0), C.S)].astype(np.float64) for k in range(n)]
            back = _through_the_file(tmp_path, raw, C.SIZE, C.CROP_TOP)
            mine = [lane for present, lane in (C.lane_of(tab, f, C.G + k, "wire") for k in range(n)) if present]
            assert len(back) == len(mine), (name, f)
            for a, b in zip(back, mine):
                assert np.array_equal(_bits(a), _bits(b)), (name, f)
    # a sweep of doubles of both forms: products of float32 coordinates, and decimals next to a tie
    r = np.random.default_rng(0)
    tx = r.uniform(-0.5, 1.5, 20000).astype(np.float32).astype(np.float64)
    vals = list(tx * 1920 / 2) + list((tx * 800 + 480) / 2) + list((r.integers(-20000, 20000, 20000) * 2 + 1) / 20.0)
    vals += [1.25 * j for j in range(-99, 100, 2)]
    vals += [0.05, 0.15, 0.25, 0.35, -0.05, -0.25, 1e15 + 0.5, 2.0 ** 52 + 1, 1e300, -1e300, 5e-324, 0.0, -0.0]
    ties = 0
    for v in vals:
        v = float(v)
        q = v * 10.0
        ties += q - math.floor(q) == 0.5
        with np.errstate(over="ignore"):
            want = np.float32(float("%.1f" % v))
        assert C.wire_value(v).view(np.uint32) == want.view(np.uint32), v
    assert ties > 500
    for v in (float("nan"), float("inf"), float("-inf")):
        assert _bits(C.wire_value(v)) == _bits(np.float32(float("%.1f" % v)))


def _matrices():
    for name, iou, lane_pts in C.matrix_cases():
        for f in range(iou.shape[0]):
            yield name, f, iou[f], lane_pts[f]
    r = np.random.default_rng(1)
    for i in range(300):
        g, l = (16, 16) if i % 3 == 0 else (int(r.integers(1, 17)), int(r.integers(1, 17)))
        iou = r.uniform(0, 1, (g, l))
        if i % 4 == 1:
            iou = np.round(iou, 2)
        if i % 4 == 2:
            iou = np.round(0.5 + iou * 0.03, 3)
        if i % 5 == 0:
            iou[r.uniform(size=(g, l)) < 0.2] = np.nan
        pts = r.choice(np.array([-1, 0, 1, 2, 7], np.int32), g + l, p=[0.1, 0.05, 0.05, 0.1, 0.7])
        yield "random", i, iou, pts


def test_matching_and_counters_equal_the_host_evaluator():
    deepest = 0
    for name, f, iou, lane_pts in _matrices():
        g = iou.shape[0]
        rows = [i for i in range(g) if lane_pts[i] >= 0]
        cols = [k for k in range(iou.shape[1]) if lane_pts[g + k] >= 0]
        sim = np.array([[0.0 if lane_pts[i] < 2 or lane_pts[g + k] < 2 else iou[i, k] for k in cols] for i in rows], np.float64)
        sim = sim.reshape(len(rows), len(cols))
        got = C.count_image(iou, lane_pts, C.THRESHOLD)
        match, tp, fp, _, fn, im = culane.count_im_pair(sim, len(rows), len(cols), C.THRESHOLD)
        assert (got["tp"], got["fp"], got["fn"]) == (tp, fp, fn), (name, f)
        assert np.float64(got["iou_im"]).view(np.uint64) == np.float64(im).view(np.uint64) or (got["iou_im"] != got["iou_im"] and im != im)
        want = np.full(g, -1, np.int32)
        for r_, c in enumerate(match):
            if c >= 0:
                want[rows[r_]] = cols[c]
        assert np.array_equal(got["anno_match"], want), (name, f)
        if len(rows) and len(cols):
            a, b, _ = C.match(sim.tolist())
            assert (a, b) == tuple(list(x) for x in culane.make_match(sim)), (name, f)
        # the cap: 16 passes per row at most, so 256 per image; the kernel's cap is four times that
        assert got["overflow"] == 0 and got["passes"] <= 256 < C.RELABEL_CAP
        deepest = max(deepest, got["passes"])
    assert deepest >= 4                                              # the sweep does relabel


def test_totals_follow_the_host_order():
    name, iou, lane_pts = C.matrix_cases()[0]
    video = np.array([0, 1, 0, 2, 1, 7], np.int32)
    got = C.count_images(iou, lane_pts, C.THRESHOLD, video, np.zeros((3, 4), np.int64), np.zeros(3))
    for v in range(3):
        tp = fp = fn = 0
        total = 0.0
        for f in np.nonzero(video == v)[0]:
            r = C.count_image(iou[f], lane_pts[f], C.THRESHOLD)
            tp += r["tp"]; fp += r["fp"]; fn += r["fn"]; total += r["iou_im"]
        assert got["totals"][v].tolist() == [tp, fp, fn, int((video == v).sum())] and got["iou_tot"][v] == total
    assert got["totals"][:, 3].sum() == 5                            # the image of row 7 is in no total


def test_library_exports_and_header_constants(built):
    names = {n for n, _, _ in _lib.declared_functions()}
    assert {"phnet_lane_eval_segments", "phnet_lane_eval_count"} <= names
    handle = ctypes.CDLL(built)
    assert hasattr(handle, "phnet_lane_eval_segments") and hasattr(handle, "phnet_lane_eval_count")
    header = open(_lib.HEADER).read()
    from phnet_amd import hip_ops
    assert f"#define PHNET_LANE_EVAL_RELABEL_CAP {C.RELABEL_CAP}\n" in header and hip_ops.LANE_EVAL_RELABEL_CAP == C.RELABEL_CAP
    assert f"#define PHNET_LANE_EVAL_MAX_LANES {hip_ops.LANE_EVAL_MAX_LANES}\n" in header
    assert f"#define PHNET_LANE_EVAL_MAX_POINTS {hip_ops.LANE_EVAL_MAX_POINTS}\n" in header
    assert hip_ops.lane_eval_rows(C.S, C.P) == C.C
    from phnet_amd.evaluation import online
    assert callable(online.LaneF1Meter) and callable(online.pack_eval_lanes)


def test_every_limit_is_refused_before_any_launch(built):
    """PHNET_ERR_ARG comes back before anything touches a device: the pointers are never followed (no GPU here)."""
    lib = _lib.lib()
    p = ctypes.c_void_p(64)                                          # non-null, never dereferenced

    def segments(F=2, G=3, L=4, S=8, P=9, mode=0, size_h=80.0, size_w=160.0, crop_top=16.0, ptrs=None):
        a = ptrs or [p] * 8
        return lib.phnet_lane_eval_segments(a[0], a[1], a[2], a[3], a[4], a[5], F, G, L, S, P, mode, size_h, size_w, crop_top, a[6], a[7], None)

    bad = [dict(G=0), dict(G=17), dict(L=0), dict(L=17), dict(S=1), dict(S=257), dict(P=1), dict(P=257), dict(F=0), dict(F=-1),
           dict(mode=2), dict(mode=-1), dict(size_h=float("inf")), dict(size_w=float("nan")), dict(crop_top=float("-inf")),
           dict(size_w=float("-inf")), dict(size_h=float("nan")),
           dict(F=(1 << 31) // (7 * 400) + 1),                       # F * (G + L) * C = 2^31 and more
           dict(F=1 << 40), dict(F=5264, G=16, L=16, S=256, P=256)]  # 5264 * 32 * 12750 > 2^31
    for kw in bad:
        assert segments(**kw) == -1, kw
    for i in range(8):
        assert segments(ptrs=[None if k == i else p for k in range(8)]) == -1, i

    def count(F=2, G=3, L=4, V=1, ptrs=None, video=None):
        a = ptrs or [p] * 10
        return lib.phnet_lane_eval_count(a[0], a[1], F, G, L, 0.5, video, V, a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], None)

    for kw in (dict(G=0), dict(G=17), dict(L=0), dict(L=17), dict(F=0), dict(F=-3), dict(F=1 << 22), dict(V=0), dict(V=-1)):
        assert count(**kw) == -1, kw
    for i in range(10):
        assert count(ptrs=[None if k == i else p for k in range(10)]) == -1, i


def test_pack_eval_lanes_raises_instead_of_truncating():
    from phnet_amd.evaluation.online import pack_eval_lanes
    lanes = [[np.zeros((3, 2)), np.ones((5, 2))], [], [np.zeros((0, 2))]]
    pts, cnt, num = pack_eval_lanes(lanes, 2, 5)
    assert tuple(pts.shape) == (3, 2, 5, 2) and cnt.tolist() == [[3, 5], [0, 0], [0, 0]] and num.tolist() == [2, 0, 1]
    assert pts[0, 1].numpy().tolist() == np.ones((5, 2)).tolist() and not pts[0, 0].any()
    with pytest.raises(ValueError):
        pack_eval_lanes(lanes, 1, 5)
    with pytest.raises(ValueError):
        pack_eval_lanes(lanes, 2, 4)
    with pytest.raises(ValueError):
        pack_eval_lanes(lanes, 17, 5)
    with pytest.raises(ValueError):
        pack_eval_lanes(lanes, 2, 257)
