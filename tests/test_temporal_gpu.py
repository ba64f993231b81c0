"""GPU side of the temporal stability evaluator: `phnet_lane_iou_groups` (csrc/lane_iou.hip) bit for bit against numpy on the
masks read back, and phnet_amd.evaluation.temporal end to end against the counts the reference's executed Python gave on the
fixture (tests/golden/temporal_tiny.json), in every batch size, through the command line, and at the OpenLane-V canvas."""
import numpy as np
import pytest
import torch

from phnet_amd.evaluation import temporal as T
from tests import temporal_cases as C

pytestmark = pytest.mark.gpu

GROUPS = [(0, 3, 3, 2), (2, 0, 0, 2), (1, 2, 4, 0), (1, 1, 1, 1), (5, 1, 5, 1), (0, 6, 0, 6), (4, 1, 1, 1)]   # (row_first, n_rows, col_first, n_cols)


@pytest.fixture(scope="module")
def ops():
    from phnet_amd import hip_ops
    return hip_ops


def _table():
    rows, total = [], 0
    for r0, nr, c0, nc in GROUPS:
        rows.append((r0, nr, c0, nc, total))
        total += nr * nc
    return np.asarray(rows, np.int32), total


def _bits(masks, width):
    m = masks.cpu().numpy().view(np.uint32)
    bits = ((m[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)
    return bits.reshape(m.shape[0], m.shape[1], -1)[:, :, :width]


def _lanes(h, w):
    """Six lanes of segments: three crossing ones, lane 3 = lane 1 again, a short one, and lane 5 entirely off the canvas."""
    rng = np.random.default_rng(h * 1000 + w)
    lanes = [[tuple(int(v) for v in rng.integers(-10, max(h, w) + 10, 4)) for _ in range(4)] for _ in range(3)]
    lanes.append(list(lanes[1]))
    lanes.append([(w // 2, h // 2, w // 2 + 3, h // 2 + 1), (0, 0, w - 1, h - 1)])
    lanes.append([(-400, -400, -300, -350)])
    return lanes


@pytest.mark.parametrize("h,w,lw", [(37, 70, 5), (64, 96, 8), (200, 333, 31)])
def test_iou_groups_bit_exact(ops, h, w, lw):
    from phnet_amd._lib import lib
    lanes = _lanes(h, w)
    segs = torch.tensor([s + (l,) for l, ss in enumerate(lanes) for s in ss], dtype=torch.int32).cuda()
    masks = ops.lane_raster(segs, len(lanes), h, w, lw)
    bits = _bits(masks, w)
    area_want = bits.reshape(len(lanes), -1).sum(1).astype(np.int64)
    assert area_want[5] == 0 and area_want[:5].min() > 0 and np.array_equal(bits[1], bits[3])
    table, total = _table()
    pairs = [(r0 + r, c0 + c) for r0, nr, c0, nc, _ in table.tolist() for r in range(nr) for c in range(nc)]
    assert len(pairs) == total == 6 + 1 + 1 + 36 + 1 and sum(1 for g in GROUPS if g[1] * g[3] and g[0] <= 1 < g[0] + g[1]) == 3
    inter = np.array([int((bits[i] & bits[j]).sum()) for i, j in pairs], np.int64)
    union = np.array([area_want[i] + area_want[j] for i, j in pairs], np.int64) - inter
    dev_table = torch.from_numpy(table).cuda()
    for scale, eps in ((1, 0.0), (3, 1e-10)):
        with np.errstate(all="ignore"):
            want = (scale * inter).astype(np.float64) / ((scale * union).astype(np.float64) + np.float64(eps))
        got, area = ops.lane_iou_groups(masks, table, w, scale, eps, want_area=True)
        got, area = got.cpu().numpy(), area.cpu().numpy()
        print(f"{h}x{w} scale {scale} eps {eps}: max |got - want| = {np.nanmax(np.abs(got - want))}, nan {int(np.isnan(got).sum())}")
        assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True)
        assert area.dtype == np.int64 and np.array_equal(area, area_want)
        assert np.array_equal(ops.lane_iou_groups(masks, table, w, scale, eps).cpu().numpy(), want, equal_nan=True)    # without `area`
        # the same call into buffers holding different garbage: every addressed element is written, nothing is accumulated
        runs = []
        for junk_f, junk_i in ((float("nan"), -1), (12345.5, 1 << 40)):
            iou_buf = torch.full((total,), junk_f, dtype=torch.float64, device="cuda")
            area_buf = torch.full((len(lanes),), junk_i, dtype=torch.int64, device="cuda")
            rc = lib().phnet_lane_iou_groups(masks.data_ptr(), len(lanes), h, w, dev_table.data_ptr(), len(table), total, scale, eps,
                                             iou_buf.data_ptr(), area_buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0
            runs.append((iou_buf.cpu().numpy(), area_buf.cpu().numpy()))
        for iou_run, area_run in runs:
            assert np.array_equal(iou_run, want, equal_nan=True) and np.array_equal(area_run, area_want)
        self_1, self_empty = 6 + 0, 6 + 1                                # the 1 x 1 groups of lane 1 and of the empty lane 5
        if eps == 0.0:
            assert got[self_1] == 1.0 and np.isnan(got[self_empty]) and got[6 + 2 + 1 * 6 + 3] == 1.0      # lanes 1 and 3 are the same
            # the existing counts on the same masks give the same quotients
            a2, i2 = ops.lane_mask_stats(masks, torch.tensor(pairs, dtype=torch.int32).cuda(), w)
            a2, i2 = a2.cpu().numpy().astype(np.float64), i2.cpu().numpy().astype(np.float64)
            with np.errstate(all="ignore"):
                old = np.array([i2[p] / (a2[i] + a2[j] - i2[p]) for p, (i, j) in enumerate(pairs)])
            assert np.array_equal(got, old, equal_nan=True)
        else:
            assert got[self_empty] == 0.0 and 0.999999 < got[self_1] <= 1.0


def test_area_only_and_empty_tables(ops):
    masks = ops.lane_raster(torch.tensor([[2, 2, 30, 20, 0], [5, 1, 5, 25, 2]], dtype=torch.int32).cuda(), 3, 32, 40, 4)
    bits = _bits(masks, 40)
    iou, area = ops.lane_iou_groups(masks, np.zeros((0, 5), np.int32), 40, want_area=True)
    assert iou.numel() == 0 and area.cpu().tolist() == [int(b.sum()) for b in bits] and area[1].item() == 0
    iou, area = ops.lane_iou_groups(masks, [[0, 0, 0, 3, 0], [1, 2, 0, 0, 0]], 40, 3, 1e-10, want_area=True)
    assert iou.numel() == 0 and area.cpu().tolist() == [int(b.sum()) for b in bits]
    assert ops.lane_iou_groups(masks, [], 40).numel() == 0


# ---------------------------------------------------------------------------------------------- the evaluator end to end
@pytest.fixture(scope="module")
def fx():
    return C.fixture()


@pytest.mark.parametrize("thr", [0.5, 0.8])
def test_evaluator_equals_the_reference_counts(fx, thr, tmp_path, capsys):
    want = fx["expected"][repr(thr)]
    h, w, lw = fx["height"], fx["width"], fx["lane_width"]
    per_video = {v: T.evaluate_frames(C.frames_of(fx, v, T), h, w, lw, thr) for v in fx["videos"]}
    C.check_against_fixture(T.summarize(per_video), want)
    anno_dir, pred_dir, names = C.write_files(fx, str(tmp_path))
    for batch in (64, 1, 3):
        C.check_against_fixture(T.evaluate(anno_dir, pred_dir, names, h, w, lw, thr, batch_frames=batch), want)
    # the command line prints (and writes) the block of the function's result
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    capsys.readouterr()
    rc = T.main(["-a", anno_dir, "-d", pred_dir, "-l", str(tmp_path / "list.txt"), "-r", str(h), "-c", str(w), "-w", str(lw),
                 "-t", repr(thr), "-o", str(tmp_path / "out.txt")])
    block = T.result_block(dict(want), "list.txt")
    assert rc == 0 and capsys.readouterr().out == block and (tmp_path / "out.txt").read_text() == block
    assert block.split("\n")[1:4] == [f"Ns: {want['Ns']}", f"Nj: {want['Nj']}", f"Nm: {want['Nm']}"]


def test_openlane_canvas_equals_the_numpy_backend():
    frames = C.synthetic_video(n_frames=6, n_lanes=4, height=640, width=960)
    got = T.evaluate_frames(frames, 640, 960, 30, 0.5)
    want = T.evaluate_frames(frames, 640, 960, 30, 0.5, ious=C.numpy_ious)
    assert got == want and len(got) == 5
    totals = [sum(t[i] for t in got) for i in range(3)]
    print("640 x 960 (Ns, Nj, Nm) per inter-frame:", got)
    assert sum(totals) == 20 and min(totals) > 0                     # every lane persists; all three outcomes occur
    # the matrices themselves, bit for bit
    R, M = T.frame_ious(frames[:2], None, 640, 960, 30)
    R2, M2 = T.frame_ious(frames[:2], None, 640, 960, 30, C.numpy_ious)
    assert all(np.array_equal(a, b) for a, b in zip(R, R2)) and np.array_equal(M[1], M2[1]) and M[0] is None
