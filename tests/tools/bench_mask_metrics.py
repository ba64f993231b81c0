"""What the mask-level video metrics cost (phnet_amd/evaluation/video.py, csrc/mask_metrics.hip): `device_counts` on 32 frame pairs of
1080 x 1920 rendered lanes (LaneRenderer label maps: 4 annotated lanes of 72 points, width 12; the prediction is the annotation moved
by a few pixels, one lane further off, one missing in every fourth frame) at the protocol's radius, ceil(0.008 * diagonal) = 18.
  * the device step: device events around `reps` calls after a warm-up, ms per call of 32 pairs and us per pair; the same for one
    pair per call (mostly launch cost).  Beside it the bytes the step must move (both masks read once) over the HBM bandwidth a copy
    achieves on this part, as a floor - the step is far from it by construction (one byte per lane in pass one).
  * HOST BASELINE, labelled as such: the restatement of the same rules on the masks copied to the host with scipy's binary_dilation
    and the 37 x 37 disk (tests/maskmetric_cases.py dilate_scipy - what the reference's db_eval_boundary does through skimage), on
    --host-pairs of the same pairs (default 2), seconds per pair; and the ratio.
  * the counts of those pairs from the device equal the restatement's (asserted), and J / F of the 32 pairs are printed.
Prints one JSON line.  --reps N (default 50 timed calls)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from phnet_amd.evaluation import video as V
from phnet_amd.overlay import LaneRenderer
from bench_stream import _arg
from bench_overlay import synthetic_polylines

H, W, PAIRS, LANES, WIDTH = 1080, 1920, 32, 4, 12
HBM_MEASURED = 6.29e12                                      # bytes / s: a float4 copy on this part


def rendered_pairs(device="cuda"):
    """(pred, gt) u8 [PAIRS, H, W] on the device."""
    r = LaneRenderer((H, W), sx=W, sy=H, oy=0, lane_width=WIDTH, device=device)
    anno = synthetic_polylines(PAIRS, 8, LANES, device)
    pred = {k: v.clone() for k, v in anno.items()}
    shift = torch.tensor([2.0, -5.0, 9.0, 40.0], device=device) / W                  # per lane, in pixels
    pred["points"][:, :LANES, :, 0] += shift[None, :, None] + torch.arange(PAIRS, device=device)[:, None, None] * (0.5 / W)
    pred["lanes_num"][::4] = LANES - 1
    return r.render(pred)["label_map"], r.render(anno)["label_map"]


def event_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def main():
    from tests import maskmetric_cases as C
    reps, host_pairs = int(_arg("--reps", 50)), int(_arg("--host-pairs", 2))
    pred, gt = rendered_pairs()
    radius = V.boundary_radius(H, W)
    for _ in range(5):
        counts = V.device_counts(pred, gt)
        V.device_counts(pred[:1], gt[:1])
    ms32 = [event_ms(lambda: V.device_counts(pred, gt), reps) for _ in range(3)]
    ms1 = [event_ms(lambda: V.device_counts(pred[:1], gt[:1]), reps) for _ in range(3)]
    k = counts.cpu().numpy()
    p_host, g_host = pred[:host_pairs].cpu().numpy(), gt[:host_pairs].cpu().numpy()
    assert np.array_equal(k[:host_pairs], C.counts(p_host, g_host, radius)), "device counts differ from the restatement"
    t0 = time.perf_counter()
    for i, (p, g) in enumerate(zip(p_host, g_host)):
        bp, bg = C.boundary_map(p), C.boundary_map(g)
        host = [(p != 0).sum(), (g != 0).sum(), ((p != 0) & (g != 0)).sum(), bp.sum(), bg.sum(),
                (bp & C.dilate_scipy(bg, radius)).sum(), (bg & C.dilate_scipy(bp, radius)).sum()]
        assert [int(v) for v in host] == k[i].tolist(), "device counts differ from scipy's"
    host_s = (time.perf_counter() - t0) / max(1, host_pairs)
    med32, med1 = sorted(ms32)[1], sorted(ms1)[1]
    moved = 2 * H * W
    out = {"workload": f"{PAIRS} pairs of {H}x{W} label maps, {LANES} lanes of width {WIDTH}, radius {radius}; {reps} timed calls, 3 runs, device events",
           "device_ms_per_call_32_pairs": {"runs": [round(x, 4) for x in ms32], "median": round(med32, 4)},
           "device_us_per_pair": round(med32 * 1e3 / PAIRS, 2),
           "device_ms_per_call_1_pair": {"runs": [round(x, 4) for x in ms1], "median": round(med1, 4)},
           "bytes_per_pair": moved, "floor_us_per_pair_6.29TBps": round(moved / HBM_MEASURED * 1e6, 3),
           "host_scipy_s_per_pair": round(host_s, 3), "host_pairs_timed": host_pairs,
           "host_over_device": round(host_s / (med32 * 1e-3 / PAIRS), 0),
           "boundary_pixels_per_pair": [int(k[:, 3].mean()), int(k[:, 4].mean())],
           "J_mean": round(float(V.jaccard(k, (H, W)).mean()), 4), "F_mean": round(float(V.boundary_f(k).mean()), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
