"""GPU side of the mask-level video metrics: `phnet_mask_metrics` (csrc/mask_metrics.hip) against the numpy / scipy restatement of
tests/maskmetric_cases.py, all seven counts, exactly - everything is integer arithmetic, so equality is the criterion and no
tolerance appears.  The restatement itself is held to the reference's executed code by tests/test_mask_metrics_cpu.py."""
import numpy as np
import pytest
import torch

from phnet_amd.evaluation import video as V
from tests import maskmetric_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from phnet_amd import hip_ops
    return hip_ops


def device(ops, pred, gt, radius):
    p, g = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.uint8)).cuda(), torch.from_numpy(np.ascontiguousarray(gt, dtype=np.uint8)).cuda()
    return ops.mask_metric_counts(p, g, radius).cpu().numpy()


def check(ops, pred, gt, radius, what=""):
    want, got = C.counts(pred, gt, radius), device(ops, pred, gt, radius)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), (what, radius, got.tolist(), want.tolist())
    return want


def test_fixture_cases(ops):
    for c in C.fixture_cases():
        k = check(ops, c["pred"], c["gt"], c["radius"], c["name"])
        assert float(V.boundary_f(k)) == c["F"] and float(V.jaccard(k, c["pred"].shape)) == c["J2"]
        assert float(V.jaccard(k, c["pred"].shape, two_class=False)) == c["J"]


@pytest.mark.parametrize("w", [1, 63, 64, 65, 70, 160, 200])
def test_ragged_last_word_and_no_wrap_between_rows(ops, w):
    """A foreground column at x = W - 1 against one at x = 0: bits past W in the last word must stay zero and a dilation must not
    reach from one row's end into the next row's start."""
    pred, gt = C.edge_columns(9, w)
    for radius in (0, 3, 66):
        check(ops, pred, gt, radius, w)


@pytest.mark.parametrize("h,w,radius", [(5, 130, 18), (1, 130, 4), (1, 1, 2), (3, 200, 127), (33, 65, 40)])
def test_heights_below_the_radius(ops, h, w, radius):
    pred, gt = C.pair(h, w, 100 + h, shift=(0, 3))
    k = check(ops, pred, gt, radius, (h, w))
    if h == 1 and w > 1:
        assert k[3] > 0                                # a single row still has s ^ e boundaries


@pytest.mark.parametrize("radius", [0, 1, 18, 63, 64, 65, 127])
def test_radii_across_word_boundaries(ops, radius):
    """Sparse points (so that a large disk does not cover everything) and blobs: shifts that cross one and two 64-bit words."""
    h, w = (40, 300) if radius == 127 else (40, 200)
    rng = np.random.default_rng(radius)
    pred, gt = (rng.random((h, w)) < 0.002).astype(np.uint8), (rng.random((h, w)) < 0.002).astype(np.uint8)
    pred[:, w - 1] = 1
    gt[:, 0] = 1
    check(ops, pred, gt, radius, "points")
    p2, g2 = C.pair(h, w, 200 + radius, shift=(2, 9))
    check(ops, p2, g2, radius, "blobs")


def test_structures_straddle_tile_seams(ops):
    """300 x 700 is larger than the LDS tile (32 rows x 512 pixels) in both directions; blobs sit on all four image borders."""
    pred, gt = C.pair(300, 700, 5, shift=(7, -13))
    for m in (pred, gt):
        assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any()
    k = check(ops, pred, gt, 18)
    assert 0 < k[5] < k[3] and 0 < k[6] < k[4]


def test_frames_are_independent_and_leading_dimensions_flatten(ops):
    h, w, radius = 37, 150, 6
    pairs = [C.pair(h, w, s, shift=(s % 5, 3 - s)) for s in range(6)]
    pred, gt = np.stack([p for p, _ in pairs]), np.stack([g for _, g in pairs])
    single = np.stack([device(ops, p, g, radius) for p, g in pairs])
    assert np.array_equal(single, C.counts(pred, gt, radius)) and len({tuple(r) for r in single.tolist()}) == 6
    assert np.array_equal(device(ops, pred[:3], gt[:3], radius), single[:3])
    got = device(ops, pred.reshape(2, 3, h, w), gt.reshape(2, 3, h, w), radius)
    assert got.shape == (2, 3, 7) and np.array_equal(got.reshape(6, 7), single)
    empty = ops.mask_metric_counts(torch.zeros(0, h, w, dtype=torch.uint8, device="cuda"), torch.zeros(0, h, w, dtype=torch.uint8, device="cuda"), 2)
    assert tuple(empty.shape) == (0, 7)
    with pytest.raises(ValueError):
        ops.mask_metric_counts(torch.zeros(2, h, w, dtype=torch.uint8, device="cuda"), torch.zeros(3, h, w, dtype=torch.uint8, device="cuda"), 2)
    with pytest.raises(ValueError):
        ops.mask_metric_counts(torch.zeros(2, h, w, dtype=torch.uint8, device="cuda"), torch.zeros(2, h, w, dtype=torch.uint8, device="cuda"), 128)


def test_every_non_zero_byte_is_foreground(ops):
    pred, gt = C.pair(40, 130, 3)
    want = C.counts(pred, gt, 4)
    for a, b in ((1, 1), (128, 255), (255, 128), (2, 77)):
        assert np.array_equal(device(ops, pred * np.uint8(a), gt * np.uint8(b), 4), want), (a, b)
    labels = np.random.default_rng(0).integers(1, 256, pred.shape).astype(np.uint8)
    assert np.array_equal(device(ops, pred * labels, gt * labels[::-1], 4), want)


def test_nothing_depends_on_what_the_buffers_held(ops):
    """Counts and workspace pre-filled with 0xFF; a second call on the same buffers; a smaller problem after a larger one."""
    pred, gt = C.pair(70, 210, 9, shift=(2, 6))
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    want = C.counts(pred, gt, 7)
    first = ops.mask_metric_counts(p, g, 7)
    ws = ops.workspace(1, p.device)
    ws.fill_(0xFF)
    out = torch.full((7,), -1, dtype=torch.int64, device="cuda")
    assert ops.mask_metric_counts(p, g, 7, out=out) is out
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(first.cpu().numpy(), want)
    ops.mask_metric_counts(p, g, 7, out=out)
    assert np.array_equal(out.cpu().numpy(), want)
    small = check(ops, pred[:20, :70], gt[:20, :70], 7)                              # the workspace now holds the larger problem's words
    assert small[3] > 0


def test_rendered_label_maps_through_the_evaluator(ops):
    """LaneRenderer.render label maps of two hand-made polyline sets -> VideoMaskEval == the restatement on the maps copied back."""
    from phnet_amd.overlay import LaneRenderer
    H, W, F, L, S = 96, 160, 3, 4, 6
    ys = np.linspace(0.95, 0.2, S)
    anno, pred = np.zeros((F, L, S, 2), np.float32), np.zeros((F, L, S, 2), np.float32)
    for f in range(F):
        for k in range(3):
            xs = 0.2 + 0.25 * k + (0.1 * (k - 1)) * (ys - 0.2) + 0.01 * f
            anno[f, k] = np.stack([xs, ys], 1)
            pred[f, k] = np.stack([xs + (0.0, 0.02, 0.08)[k] + 0.01 * f, ys], 1)       # on the lane, a few pixels off, far off
    count = np.zeros((F, L), np.int32)
    count[:, :3] = S
    num_anno, num_pred = np.full(F, 3, np.int32), np.array([3, 2, 0], np.int32)       # the last frame has no prediction
    r = LaneRenderer((H, W), sx=W, sy=H, oy=0, lane_width=5)
    dev = lambda *a: [torch.from_numpy(x).cuda() for x in a]                           # noqa: E731
    maps = []
    for pts, num in ((pred, num_pred), (anno, num_anno)):
        p, c, n = dev(pts, count, num)
        maps.append(r.render(dict(points=p, count=c, lanes_num=n))["label_map"])
    assert maps[0].dtype == torch.uint8 and tuple(maps[0].shape) == (F, H, W) and int(maps[0].max()) == 3
    ev = V.VideoMaskEval()
    ev.update("clip_a", maps[0][:2], maps[1][:2])
    ev.update("clip_a", maps[0][2:], maps[1][2:])
    ev.update("clip_b", maps[0][1:2], maps[1][1:2])
    got = ev.summary()
    radius = V.boundary_radius(H, W)
    assert radius == 2
    k = C.counts(maps[0].cpu().numpy(), maps[1].cpu().numpy(), radius)
    j, f = V.jaccard(k, (H, W)), V.boundary_f(k)
    assert 0.1 < f[0] < 1 and f[2] == 0.0 and k[2, 3] == 0 and k[2, 4] > 0
    assert got["per_video"]["clip_a"] == dict(J=float(np.sum(j) / 3), F=float(np.sum(f) / 3), frames=3)
    assert got["per_video"]["clip_b"] == dict(J=float(j[1]), F=float(f[1]), frames=1)
    assert got["J"] == float(np.sum([got["per_video"][v]["J"] for v in ("clip_a", "clip_b")]) / 2)


def test_command_line_scores_lines_files(ops, tmp_path, capsys):
    """The .lines.txt route: both sides drawn by phnet_lane_raster into one mask per frame, scored, printed and written as JSON;
    against the restatement on masks drawn by the project's CPU rasteriser."""
    import json
    from oracle import culane_cpu as O
    H, W, LW = 60, 100, 7
    lanes = {"v0/000": ([[(10.5, 55.0), (30.2, 20.0), (35.0, 5.0)], [(70.0, 58.0), (60.0, 10.0)]], [[(12.5, 55.0), (33.2, 20.0)], [(90.0, 58.0), (95.0, 10.0)]]),
             "v0/001": ([[(20.0, 50.0), (40.0, 8.0)]], []),
             "v1/000": ([[(50.0, 59.0), (50.0, 0.0)]], [[(53.0, 59.0), (52.0, 0.0)]])}
    for side in ("anno", "pred"):
        for v in ("v0", "v1"):
            (tmp_path / side / v).mkdir(parents=True)
    for name, (anno, pred) in lanes.items():
        for side, ls in (("anno", anno), ("pred", pred)):
            (tmp_path / side / (name + ".lines.txt")).write_text("".join(" ".join("%.2f %.2f" % p for p in l) + " \n" for l in ls))
    (tmp_path / "list.txt").write_text("\n".join(lanes) + "\n")
    out = tmp_path / "out.json"
    assert V.main(["-a", str(tmp_path / "anno"), "-d", str(tmp_path / "pred"), "-l", str(tmp_path / "list.txt"), "-r", str(H), "-c", str(W),
                   "-w", str(LW), "-b", "2", "-o", str(out)]) == 0
    res = json.loads(out.read_text())

    def mask(ls):
        m = np.zeros((H, W), bool)
        for l in ls:
            q = [(int(x), int(y)) for x, y in l]
            m |= O.raster_lane([a + b for a, b in zip(q[:-1], q[1:])], H, W, LW)
        return m

    k = C.counts(np.stack([mask(p) for _, p in lanes.values()]), np.stack([mask(a) for a, _ in lanes.values()]), V.boundary_radius(H, W))
    j, f = V.jaccard(k, (H, W)), V.boundary_f(k)
    assert k[0, 0] > 0 and k[1, 0] == 0 and 0 < f[0] < 1
    assert res["per_video"]["v0"] == dict(J=float(np.sum(j[:2]) / 2), F=float(np.sum(f[:2]) / 2), frames=2)
    assert res["per_video"]["v1"] == dict(J=float(j[2]), F=float(f[2]), frames=1)
    assert "v0: J" in capsys.readouterr().out


def test_graph_capture_and_replay(ops):
    a, b = C.pair(50, 140, 21, shift=(3, 4)), C.pair(50, 140, 22, shift=(-2, 8))
    p, g = torch.from_numpy(a[0]).cuda(), torch.from_numpy(a[1]).cuda()
    out = torch.full((7,), -1, dtype=torch.int64, device="cuda")
    ops.mask_metric_counts(p, g, 5, out=out)                                         # warm-up: the workspace exists
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.mask_metric_counts(p, g, 5, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), C.counts(a[0], a[1], 5))
    p.copy_(torch.from_numpy(b[0])); g.copy_(torch.from_numpy(b[1]))
    out.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    want = C.counts(b[0], b[1], 5)
    assert np.array_equal(out.cpu().numpy(), want) and not np.array_equal(want, C.counts(a[0], a[1], 5))
