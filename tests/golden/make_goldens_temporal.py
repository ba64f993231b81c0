"""Golden counts of the temporal stability metric: runs the REFERENCE's own evaluation/evalTemporalOLV2.py (read-only checkout
at /root/reference, loaded by path, unmodified) on small synthetic videos and stores the lane texts with the counts it gives.
Build container only:  python tests/golden/make_goldens_temporal.py   -> tests/golden/temporal_tiny.json

Stand-ins (none of them is in this image): tqdm, p_tqdm, shapely.geometry and libs.dataset.openlane.utils are empty shells
(nothing on the official num_t = 1 path calls them), and a `cv2` whose line(img, p1, p2, color, thickness) sets all three
channels of the pixels oracle.culane_cpu.raster_lane sets for that segment - the project's rasterisation rule; parity against
OpenCV's scan conversion is unpinned (oracle/culane_cpu.py).  `settings()` holds its author's paths and is bypassed: lane_width,
official, num_t, iou_threshold, shape, pred_dir, anno_dir are set on the instance and `mainMetric` is called per video.

Content: canvas 96 x 160, lane width 12, thresholds 0.5 and 0.8; three videos of 8 - 12 frames and one of a single frame; lanes
appear, disappear and jump in the annotation; predictions are dropped, shifted by more than a lane width, shifted by a few
pixels (IoU between the two thresholds) and spurious; one frame has no predictions, one has no annotations.

Two conditions are asserted, so that the fixture pins what it is meant to pin: each of Ns, Nj, Nm is >= 2 at threshold 0.5, and
every IoU of an assigned pair (all of them are recorded where the reference calls linear_sum_assignment: a superset of those
that reach a threshold comparison) is at least 0.02 away from both thresholds - a last-bit difference in FITPACK between scipy
builds cannot flip a count."""
import importlib.util
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np

from oracle import culane_cpu as O

REF_FILE = "/root/reference/evaluation/evalTemporalOLV2.py"
H, W, LANE_WIDTH = 96, 160, 12
THRESHOLDS = (0.5, 0.8)
MARGIN = 0.02
SEED = 21


def _cv2_line(img, p1, p2, color=(255, 255, 255), thickness=1):
    m = O.raster_lane([(int(p1[0]), int(p1[1]), int(p2[0]), int(p2[1]))], img.shape[0], img.shape[1], int(thickness))
    img[m] = color
    return img


def load_reference():
    shells = {"cv2": dict(line=_cv2_line), "tqdm": dict(tqdm=lambda x, *a, **k: x), "p_tqdm": dict(t_map=None, p_map=None),
              "shapely": {}, "shapely.geometry": dict(LineString=None, Polygon=None),
              "libs": {}, "libs.dataset": {}, "libs.dataset.openlane": {},
              "libs.dataset.openlane.utils": dict(load_pickle=None, save_pickle=None)}
    saved = {k: sys.modules.get(k) for k in shells}
    for name, attrs in shells.items():
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        if name in ("shapely", "libs", "libs.dataset", "libs.dataset.openlane"):
            mod.__path__ = []
        sys.modules[name] = mod
    try:
        spec = importlib.util.spec_from_file_location("ref_eval_temporal", REF_FILE)
        ref = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ref)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return ref


# ---------------------------------------------------------------------------------------------- synthetic videos
def lane_points(x_bottom, slope, bend, n):
    ys = np.linspace(H - 6, 14, n)
    s = (ys[0] - ys) / (ys[0] - ys[-1])
    return [(x_bottom + slope * v + bend * v * v, y) for v, y in zip(s, ys)]


def text_of(lanes):
    return "".join(" ".join("%.2f %.2f" % p for p in lane) + " \n" for lane in lanes)


def make_video(rng, n_frames, tracks, no_pred_frame=None, no_anno_frame=None):
    """tracks: (x_bottom, slope, bend, first frame, last frame, jump frame or None).  -> [(anno text, pred text)]"""
    frames = []
    drift = [0.0] * len(tracks)
    for t in range(n_frames):
        anno, pred = [], []
        for k, (x0, slope, bend, first, last, jump) in enumerate(tracks):
            drift[k] += float(rng.integers(0, 2))                                  # 0 or 1 pixel per frame: stays persistent
            if jump is not None and t == jump:
                drift[k] += 9.0                                                    # more than half a lane: not persistent
            if not first <= t <= last:
                continue
            lane = lane_points(x0 + drift[k], slope, bend, int(rng.integers(4, 8)))
            anno.append(lane)
            mode = rng.choice(["good", "good", "good", "near", "far", "drop"])
            if mode == "drop":
                continue
            shift = {"good": float(rng.integers(0, 2)), "near": float(rng.integers(2, 4)), "far": float(rng.integers(14, 22))}[mode]
            pred.append([(x + shift, y) for x, y in lane_points(x0 + drift[k], slope, bend, int(rng.integers(4, 8)))])
        if rng.random() < 0.3:                                                     # a spurious detection
            pred.append(lane_points(float(rng.integers(8, W - 8)), float(rng.integers(-50, 50)), 0.0, 5))
        if t == no_pred_frame:
            pred = []
        if t == no_anno_frame:
            anno = []
        order = rng.permutation(len(pred))
        frames.append((text_of(anno), text_of([pred[i] for i in order])))
    return frames


def make_videos(seed):
    rng = np.random.default_rng(seed)
    return {
        "seq_a": make_video(rng, 10, [(30, 25, 4, 0, 9, None), (78, 4, -6, 0, 6, None), (128, -24, 3, 2, 9, 5)], no_pred_frame=4),
        "seq_b": make_video(rng, 12, [(24, 30, 0, 0, 11, None), (66, 8, 5, 3, 11, None), (104, -10, -4, 0, 8, 6), (140, -30, 0, 1, 10, None)],
                            no_anno_frame=7),
        "seq_c": make_video(rng, 8, [(50, 14, 6, 0, 7, 3), (110, -16, -5, 0, 7, None)]),
        "seq_d": make_video(rng, 1, [(40, 10, 0, 0, 0, None), (120, -10, 0, 0, 0, None)]),
    }


# ---------------------------------------------------------------------------------------------- the reference on them
def run_reference(ref, videos, threshold, assigned):
    datalist = {v: [f"{v}/{t:03d}" for t in range(len(frames))] for v, frames in videos.items()}
    with tempfile.TemporaryDirectory() as tmp:
        for v, frames in videos.items():
            for side in ("anno", "pred"):
                os.makedirs(os.path.join(tmp, side, v))
            for name, (anno, pred) in zip(datalist[v], frames):
                open(os.path.join(tmp, "anno", name + ".lines.txt"), "w").write(anno)
                open(os.path.join(tmp, "pred", name + ".lines.txt"), "w").write(pred)
        ev = ref.LaneEval_Temporal(cfg=types.SimpleNamespace(num_t=1))
        ev.lane_width, ev.official, ev.num_t, ev.iou_threshold = LANE_WIDTH, True, 1, threshold
        ev.shape = (H, W, 3)
        ev.pred_dir, ev.anno_dir = os.path.join(tmp, "pred"), os.path.join(tmp, "anno")
        solve = ref.linear_sum_assignment

        def recording(cost):
            rows, cols = solve(cost)
            assigned.extend((1 - np.asarray(cost)[rows, cols]).tolist())
            return rows, cols

        ref.linear_sum_assignment = recording
        try:
            return {v: [[int(x) for x in trio] for trio in ev.mainMetric(datalist, v)] for v in videos}
        finally:
            ref.linear_sum_assignment = solve


def totals(per_video):
    ns = sum(t[0] for v in per_video.values() for t in v)
    nj = sum(t[1] for v in per_video.values() for t in v)
    nm = sum(t[2] for v in per_video.values() for t in v)
    n = ns + nj + nm
    return {"Ns": ns, "Nj": nj, "Nm": nm, "Rs": float(ns) / n, "Rj": float(nj) / n, "Rm": float(nm) / n}


def main():
    ref = load_reference()
    videos = make_videos(SEED)
    expected, assigned = {}, []
    for thr in THRESHOLDS:
        per_video = run_reference(ref, videos, thr, assigned)
        expected[repr(thr)] = dict(totals(per_video), per_video=per_video,
                                   video_totals={v: [sum(t[i] for t in trios) for i in range(3)] for v, trios in per_video.items()})
        print(thr, {k: v for k, v in expected[repr(thr)].items() if k != "per_video"})
    at_half = expected[repr(0.5)]
    assert min(at_half["Ns"], at_half["Nj"], at_half["Nm"]) >= 2, at_half
    gap = min(abs(v - thr) for v in assigned for thr in THRESHOLDS)
    print("assigned IoUs:", len(assigned), "closest to a threshold:", gap)
    assert gap >= MARGIN, gap
    assert [len(f) for f in videos.values()] == [10, 12, 8, 1]
    out = {"height": H, "width": W, "lane_width": LANE_WIDTH, "thresholds": list(THRESHOLDS),
           "videos": {v: [{"name": f"{v}/{t:03d}", "anno": a, "pred": p} for t, (a, p) in enumerate(frames)] for v, frames in videos.items()},
           "expected": expected}
    with open(os.path.join(HERE, "temporal_tiny.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
