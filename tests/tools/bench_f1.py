"""What validation F1 on the device costs (phnet_amd/evaluation/online.py, csrc/lane_eval.hip): one `LaneF1Meter.update` of 64
images at 1280 x 1920 with 4 annotated and 4 predicted lanes per image (annotations of 20 points, predictions of 36, lane width 30).
  * the update: device events around `reps` eager calls after a warm-up, and around replays of the update captured in a hipGraph;
    ms per call of 64 images, and the five stages (memset, segments, raster, IoU, count) timed one by one;
  * PARENT'S PATH, labelled as such, on the same lanes already parsed (no files written or read, which favours it):
    `culane.similarity_matrices` (host splines, upload, raster, pair counts, download) + `culane.count_im_pair` per image, wall clock
    per 64 images; tp / fp / fn and the IoU sum of the two paths are asserted equal;
  * the cost of the fixed-stride segment table: the same lanes in a meter sized for annotations of 256 points (12 750 rows per lane
    instead of 3 150), where most raster workgroups find lane -1 and return.
Prints one JSON line.  --reps N (default 20 timed calls)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from phnet_amd import hip_ops as K
from phnet_amd.evaluation import culane
from phnet_amd.evaluation.online import LaneF1Meter, pack_eval_lanes
from bench_stream import _arg
from bench_mask_metrics import event_ms

H, W, IMAGES, LANES, S, GT_POINTS, WIDTH, THRESHOLD, SIZE, CROP_TOP = 1280, 1920, 64, 4, 36, 20, 30, 0.5, (800, 1920), 480


def synthetic_lanes(seed=0):
    """(annotations [image][lane] float32 [20,2] in evaluator coordinates, predictions dict of normalised polylines [64,4,36,2])."""
    r = np.random.default_rng(seed)
    anno, points = [], np.zeros((IMAGES, LANES, S, 2), np.float32)
    for f in range(IMAGES):
        lanes = []
        for i in range(LANES):
            ys = np.linspace(1270, 520, GT_POINTS)
            xs = 250 + 420 * i + np.cumsum(r.normal(0, 12, GT_POINTS))
            lanes.append((np.rint(np.stack([xs, ys], 1) * 2) / 2).astype(np.float32))
            py = np.linspace(ys[0], ys[-1], S)
            px = np.interp(-py, -ys, xs) + r.normal(0, 1.0) + (25.0 if (f + i) % 7 == 0 else 2.0)        # one in seven is a miss
            points[f, i] = np.stack([px / (SIZE[1] / 2), (py * 2 - CROP_TOP) / SIZE[0]], 1)[::-1]           # last point first
        anno.append(lanes)
    pred = dict(points=torch.from_numpy(points).cuda(), count=torch.full((IMAGES, LANES), S, dtype=torch.int32, device="cuda"),
                lanes_num=torch.full((IMAGES,), LANES, dtype=torch.int32, device="cuda"))
    return anno, pred


def stages(meter, pred, gt):
    f, g, l = IMAGES, meter.max_gt_lanes, meter.max_lanes
    n = f * (g + l)
    masks, out = meter._masks[:n], dict(segs=meter._segs[:n], lane_pts=meter._lane_pts[:f])
    rows = {k: v[:f] for k, v in meter._rows.items()}
    return {"memset": lambda: masks.zero_(),
            "segments": lambda: K.lane_eval_segments(pred["points"], pred["count"], pred["lanes_num"], *gt, meter.mode, meter.size,
                                                     meter.crop_top, out=out),
            "raster": lambda: K.lane_raster(out["segs"].view(-1, 5), n, H, W, WIDTH, masks=masks),
            "iou": lambda: K.lane_iou_groups_device(masks, meter._groups[:f], f * g * l, W, meter._iou[:f]),
            "count": lambda: K.lane_eval_count(meter._iou[:f], out["lane_pts"], g, THRESHOLD, meter._totals, meter._iou_tot,
                                               meter._overflow, out=rows)}


def measure(max_gt_points, anno, pred, reps):
    meter = LaneF1Meter(H, W, WIDTH, THRESHOLD, size=SIZE, crop_top=CROP_TOP, max_images=IMAGES, max_gt_lanes=LANES,
                        max_gt_points=max_gt_points, max_lanes=LANES, n_offsets=S)
    gt = [t.cuda() for t in pack_eval_lanes(anno, LANES, max_gt_points)]
    update = lambda: meter.update(pred, *gt)
    for _ in range(3):
        update()
    eager = sorted(event_ms(update, reps) for _ in range(3))[1]
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        update()
    graph.replay()
    replay = sorted(event_ms(graph.replay, reps) for _ in range(3))[1]
    per_stage = {k: round(sorted(event_ms(fn, reps) for _ in range(3))[1], 4) for k, fn in stages(meter, pred, gt).items()}
    meter.reset()
    update()
    res = meter.compute()
    return dict(rows_per_lane=meter.rows_per_lane, raster_workgroups=IMAGES * 2 * LANES * meter.rows_per_lane,
                eager_ms=round(eager, 4), graph_replay_ms=round(replay, 4), stages_ms=per_stage), res, meter.iou_sum()


def parent_path(anno, pred, reps):
    """similarity_matrices + count_im_pair on the lanes the evaluator would have read back from the files."""
    from tests import f1_cases as C
    t = dict(points=pred["points"].cpu().numpy(), count=pred["count"].cpu().numpy(), lanes_num=pred["lanes_num"].cpu().numpy(),
             gt_points=np.zeros((IMAGES, 1, 2, 2), np.float32), gt_count=np.zeros((IMAGES, 1), np.int32), gt_num=np.zeros(IMAGES, np.int32))
    images = [(anno[f], [C.lane_of(t, f, 1 + k, "wire", SIZE, CROP_TOP)[1] for k in range(LANES)]) for f in range(IMAGES)]
    def run():
        tp = fp = fn = 0
        iou = 0.0
        sims = culane.similarity_matrices(images, H, W, WIDTH)
        for (a, d), sim in zip(images, sims):
            _, x, y, _, z, w = culane.count_im_pair(sim, len(a), len(d), THRESHOLD)
            tp += x; fp += y; fn += z; iou += w
        return tp, fp, fn, iou
    run()
    times = []
    for _ in range(max(3, reps // 4)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run()
        times.append((time.perf_counter() - t0) * 1e3)
    return sorted(times)[len(times) // 2], out


def main():
    reps = int(_arg("--reps", 20))
    anno, pred = synthetic_lanes()
    tight, res, iou_sum = measure(GT_POINTS, anno, pred, reps)
    host_ms, (tp, fp, fn, iou) = parent_path(anno, pred, reps)
    assert (res["tp"], res["fp"], res["fn"]) == (tp, fp, fn) and iou_sum == iou, "the device update differs from the parent's path"
    wide, res_wide, iou_wide = measure(256, anno, pred, reps)
    assert (res_wide["tp"], res_wide["fp"], res_wide["fn"]) == (tp, fp, fn) and iou_wide == iou
    out = {"workload": f"{IMAGES} images of {H}x{W}, {LANES}+{LANES} lanes ({GT_POINTS}-point annotations, {S}-point predictions), width {WIDTH}; "
                       f"{reps} timed calls, median of 3 runs, device events",
           "update_P20": tight, "update_P256": wide,
           "parent_similarity_matrices_plus_count_ms": round(host_ms, 2),
           "parent_over_update_eager": round(host_ms / tight["eager_ms"], 1),
           "images_per_s_eager": round(IMAGES / (tight["eager_ms"] * 1e-3)),
           "tp_fp_fn": [tp, fp, fn], "miou": res["miou"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
