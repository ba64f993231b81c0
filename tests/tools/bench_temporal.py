"""What the temporal stability evaluator costs (phnet_amd/evaluation/temporal.py, csrc/lane_iou.hip): one video of 64 frames
with 4 annotated + 4 predicted lanes at the OpenLane-V canvas 640 x 960, lane width 30 (tests/temporal_cases.synthetic_video).
  * the IoU step on the SAME masks (512 lanes drawn = what one batch of the evaluator holds; 64 R matrices and 63 M matrices
    of 4 x 4 = 2032 entries): `phnet_lane_iou_groups` (one launch, matrices out) against the path the CULane evaluator
    uses, `phnet_lane_mask_stats` on the pair list of the same entries (+ two zero fills) followed by the copy back and the
    host loops that assemble the matrices.  Device time = device events around `launches` back-to-back calls (it includes
    the launch gaps; it is not a profiler's kernel time), three alternated rounds; the host assembly is timed by the host clock.
  * `evaluate_frames` end to end, frames per second, three runs after a warm-up; and where the time goes: host spline + segments,
    device (upload, raster, IoU, copy back: host clock around a synchronise), host matching + counting.
Prints one JSON line.  --launches N (default 200)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from phnet_amd import hip_ops as K
from phnet_amd.evaluation import temporal as T
from tests import temporal_cases as C

H, W, LW, FRAMES, ROUNDS = 640, 960, 30, 64, 3


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def _events(fn, launches):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches * 1e3


def _spread(v):
    return {"median": round(float(np.median(v)), 2), "min": round(float(min(v)), 2), "max": round(float(max(v)), 2)}


def main():
    launches = int(_arg("--launches", 200))
    frames = C.synthetic_video(n_frames=FRAMES, n_lanes=4, height=H, width=W)
    captured = {}

    def capture(segments, groups, h, w, lw):
        captured["segments"], captured["groups"] = segments, np.asarray(groups, np.int32)
        return T.device_ious(segments, groups, h, w, lw)

    T.frame_ious(frames, None, H, W, LW, capture)                    # also the warm-up of both kernels
    segments, groups = captured["segments"], captured["groups"]
    rows = np.concatenate([np.concatenate([s, np.full((len(s), 1), l, np.int32)], axis=1) for l, s in enumerate(segments)])
    segs = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()
    masks = K.lane_raster(segs, len(segments), H, W, LW)
    table, n_entries = K.check_iou_groups(groups, len(segments))
    pairs_host = [(r0 + r, c0 + c) for r0, nr, c0, nc, _ in table.tolist() for r in range(nr) for c in range(nc)]
    pairs = torch.tensor(pairs_host, dtype=torch.int32).cuda()
    dev_table = torch.from_numpy(table).cuda()
    iou = torch.empty(n_entries, dtype=torch.float64, device="cuda")
    area = torch.zeros(len(segments), dtype=torch.int64, device="cuda")
    inter = torch.zeros(n_entries, dtype=torch.int64, device="cuda")
    lib, stream = K.lib(), torch.cuda.current_stream().cuda_stream

    def new():
        K.check(lib.phnet_lane_iou_groups(masks.data_ptr(), len(segments), H, W, dev_table.data_ptr(), len(table), n_entries, T.SCALE,
                                          T.EPS, iou.data_ptr(), None, stream), "phnet_lane_iou_groups")

    def old():
        area.zero_(); inter.zero_()
        K.check(lib.phnet_lane_mask_stats(masks.data_ptr(), len(segments), H, W, pairs.data_ptr(), n_entries, area.data_ptr(),
                                          inter.data_ptr(), stream), "phnet_lane_mask_stats")

    def assemble():
        a, i = area.cpu().numpy(), inter.cpu().numpy()
        out, p = [], 0
        for r0, nr, c0, nc, _ in table.tolist():
            m = np.zeros((nr, nc))
            for r in range(nr):
                for c in range(nc):
                    m[r, c] = float(3 * i[p]) / (float(3 * (a[r0 + r] + a[c0 + c] - i[p])) + 1e-10)
                    p += 1
            out.append(m)
        return out

    us_new, us_old, ms_asm = [], [], []
    for _ in range(ROUNDS):
        us_new.append(_events(new, launches)); us_old.append(_events(old, launches))
        t = time.perf_counter(); mats = assemble(); ms_asm.append((time.perf_counter() - t) * 1e3)
    new(); torch.cuda.synchronize()
    same = bool(np.array_equal(np.concatenate([m.reshape(-1) for m in mats]), iou.cpu().numpy()))
    words = H * ((W + 31) // 32)
    # end to end
    T.evaluate_frames(frames, H, W, LW, 0.5)
    fps = []
    for _ in range(ROUNDS):
        t = time.perf_counter(); res = T.evaluate_frames(frames, H, W, LW, 0.5); fps.append(FRAMES / (time.perf_counter() - t))
    split = {"spline_segments_ms": 0.0, "device_ms": 0.0}

    def timed_device(segments, groups, h, w, lw):
        torch.cuda.synchronize(); t = time.perf_counter()
        out = T.device_ious(segments, groups, h, w, lw)
        torch.cuda.synchronize(); split["device_ms"] += (time.perf_counter() - t) * 1e3
        return out

    t = time.perf_counter(); T.evaluate_frames(frames, H, W, LW, 0.5, ious=timed_device); total_ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    for anno, pred in frames:
        for lane in list(anno) + list(pred):
            T.lane_segments(T.lane_polyline(lane))
    split["spline_segments_ms"] = (time.perf_counter() - t) * 1e3                   # one batch: no carried lanes to redraw
    split["matching_counting_ms"] = total_ms - split["device_ms"] - split["spline_segments_ms"]
    print(json.dumps({
        "workload": f"temporal evaluator, {FRAMES} frames x (4 + 4) lanes, {H}x{W}, lane width {LW}; {len(segments)} masks of {words} words, "
                    f"{len(table)} matrices, {n_entries} entries; {launches} launches per round, {ROUNDS} alternated rounds",
        "iou_groups_us_per_launch": _spread(us_new), "mask_stats_plus_zero_fills_us_per_launch": _spread(us_old),
        "host_assembly_after_mask_stats_ms": _spread(ms_asm), "matrices_equal": same,
        "mask_bytes_read_per_launch_iou_groups": 2 * n_entries * words * 4,
        "evaluate_frames_fps": _spread(fps), "evaluate_frames_ms": round(total_ms, 1),
        "split_ms": {k: round(v, 1) for k, v in split.items()}, "counts": [sum(t[i] for t in res) for i in range(3)]}))


if __name__ == "__main__":
    main()
