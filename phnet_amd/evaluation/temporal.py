"""Temporal stability of video lane detection, the other half of the OpenLane-V protocol: `LaneEval_Temporal` of
evaluation/evalTemporalOLV2.py for num_t = 1 and official = True (what every shipped options file sets), with the pixel work
on the GPU.

    python -m phnet_amd.evaluation.temporal -a ANNO_DIR -d PRED_DIR -l LIST -r HEIGHT -c WIDTH -w 30 -t 0.5 [-o OUT] [-b BATCH_FRAMES]

For every annotated lane that persists from frame t-1 to frame t (a pair of the optimal assignment between the two frames'
annotations with IoU > threshold) the metric asks whether it was detected in both frames (stable, Ns), in exactly one
(flicker, Nj) or in neither (missing, Nm); Rs, Rj, Rm are the shares.  OpenLane-V scores on a 640 x 960 canvas
(options4OL.py:110-111) with lanes 30 pixels wide.

Per frame the reference interpolates and draws every lane up to three times on full three-channel canvases and counts pixels
on the host (cv2 + numpy).  Here every lane of a batch of frames is interpolated once and rasterised once into a bit mask in
HBM (`phnet_lane_raster`), and the IoU matrices R_t[anno_t, pred_t] and M_t[anno_t, anno_t-1] of the whole batch come out of
one more launch (`phnet_lane_iou_groups`, scale = 3 and eps = 1e-10: the reference sums the three channels of its canvases,
:26-35).  Spline (scipy splprep / splev), assignment (scipy linear_sum_assignment) and the counters are host arithmetic exactly
as the reference calls them.  `device_ious` is the only device step and has no CPU fallback: without the HIP library it raises;
everything downstream takes the matrices (or a replacement for that one function) and runs anywhere.

The rasterisation rule is the project's own (pixel centre within lane_width / 2 of the segment between the truncated end
points - include/phnet_hip.h, oracle/culane_cpu.py); parity against cv2.line stays unpinned, as for the CULane evaluator.
Differences from the reference, all on inputs it cannot score: a lane with fewer than two DISTINCT points has no pixels (the
reference raises in splprep); end points are clamped to +-8192; Rs / Rj / Rm are NaN when no lane persists anywhere (the
reference divides by zero); num_t != 1 raises ValueError and the shapely ("continuous") IoU is not built.
"""
import os
import sys
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

COORD_LIMIT = 1 << 13
SCALE, EPS = 3, 1e-10                  # three channels per pixel, `eps` of discrete_cross_iou (:26-35)
Lane = List[Tuple[float, float]]       # points as the reference holds them: hashable (x, y) pairs


# ---------------------------------------------------------------------------------------------- files (:95-107)
def lanes_from_text(text: str) -> List[Lane]:
    """The lanes of one .lines.txt text (for instance `generate_lane.format_pred_lines(...)`): whitespace-separated floats
    per line, paired into points; lanes with fewer than two points are dropped (an odd count raises, as the reshape there)."""
    lanes = []
    for line in text.splitlines():
        vals = [float(tok) for tok in line.split()]
        if len(vals) % 2:
            raise ValueError("a lane line holds an odd number of coordinates")
        lane = [(vals[i], vals[i + 1]) for i in range(0, len(vals), 2)]
        if len(lane) >= 2:
            lanes.append(lane)
    return lanes


def load_lanes(path: str) -> List[Lane]:
    """load_culane_img_data; a missing file is a frame without lanes."""
    try:
        with open(path, "r") as fh:
            return lanes_from_text(fh.read())
    except OSError:
        return []


# ---------------------------------------------------------------------------------------------- spline and segments (:50-56, :17-23)
def interp(points: Sequence, n: int = 5) -> np.ndarray:
    """:50-56: the interpolating B-spline through the points (degree min(3, len - 1), scipy's chord-length parameter `u`),
    evaluated at (len - 1) * n + 1 evenly spaced parameters -> [.., 2] float64."""
    from scipy.interpolate import splev, splprep
    x = [p[0] for p in points]
    y = [p[1] for p in points]
    tck, u = splprep([x, y], s=0, t=n, k=min(3, len(points) - 1))
    u = np.linspace(0., 1., num=(len(u) - 1) * n + 1)
    return np.array(splev(u, tck)).T


def lane_polyline(lane: Sequence) -> np.ndarray:
    """`interp(list(dict.fromkeys(lane)), n=5)` as every caller there has it; fewer than two distinct points: no poly-line."""
    pts = list(dict.fromkeys((float(p[0]), float(p[1])) for p in lane))
    if len(pts) < 2:
        return np.zeros((0, 2), np.float64)
    return interp(pts, n=5)


def lane_segments(poly: np.ndarray) -> np.ndarray:
    """[s, 4] int32 end points (x0, y0, x1, y1) of the cv2.line calls of draw_lane (:17-23): `astype(np.int32)` truncates
    toward zero (not cvRound); clamped to +-8192, the raster kernel's limit."""
    p = np.asarray(poly, dtype=np.float64).reshape(-1, 2)
    p = np.where(np.isnan(p), 0.0, p)
    q = np.trunc(np.clip(p, -COORD_LIMIT, COORD_LIMIT)).astype(np.int32)
    if len(q) < 2:
        return np.zeros((0, 4), np.int32)
    return np.ascontiguousarray(np.concatenate([q[:-1], q[1:]], axis=1))      # (the spline's points arrive transposed)


# ---------------------------------------------------------------------------------------------- IoU matrices
def device_ious(segments: Sequence[np.ndarray], groups: np.ndarray, height: int, width: int, lane_width: int,
                device="cuda") -> np.ndarray:
    """THE device step: `segments[l]` [s, 4] int32 of lane l, `groups` [G, 5] (include/phnet_hip.h) -> float64 [n_entries],
    every entry 3 I / (3 U + 1e-10) of the drawn lanes.  One raster launch and one IoU launch, one copy back."""
    import torch
    from .. import hip_ops as K
    table, n_entries = K.check_iou_groups(groups, len(segments))
    if n_entries == 0:
        return np.zeros(0, np.float64)
    rows = [np.concatenate([s, np.full((len(s), 1), l, np.int32)], axis=1) for l, s in enumerate(segments)]
    segs = torch.from_numpy(np.ascontiguousarray(np.concatenate(rows, axis=0), dtype=np.int32)).to(torch.device(device))
    masks = K.lane_raster(segs, len(segments), height, width, lane_width)
    return K.lane_iou_groups(masks, table, width, SCALE, EPS).cpu().numpy()


def frame_ious(frames: Sequence, carry: Optional[Sequence], height: int, width: int, lane_width: int,
               ious: Callable = device_ious):
    """frames: [(anno_lanes, pred_lanes)] of consecutive frames, `carry` the annotated lanes of the frame before them (None at
    the start of a video) -> (R, M): R[t] [anno_t][pred_t] (culane_metric2 :79-93) and M[t] [anno_t][anno_t-1]
    (matching_lane_instance :306-326; M[0] is None without `carry`), float64.  Every lane is interpolated and drawn once."""
    segments, groups, shapes = [], [], []
    total = 0

    def add(lanes):
        first = len(segments)
        segments.extend(lane_segments(lane_polyline(lane)) for lane in lanes)
        return first, len(lanes)

    prev = add(carry) if carry is not None else None
    for anno, pred in frames:
        a, p = add(anno), add(pred)
        per_frame = [(a, p)] + ([(a, prev)] if prev is not None else [])
        for (r0, nr), (c0, nc) in per_frame:
            groups.append((r0, nr, c0, nc, total))
            total += nr * nc
        shapes.append(per_frame)
        prev = a
    flat = ious(segments, np.asarray(groups, np.int32).reshape(-1, 5), height, width, lane_width)
    assert len(flat) == total
    R, M, g = [], [], 0
    for per_frame in shapes:
        mats = []
        for (_, nr), (_, nc) in per_frame:
            first = groups[g][4]
            mats.append(np.asarray(flat[first:first + nr * nc], np.float64).reshape(nr, nc))
            g += 1
        R.append(mats[0])
        M.append(mats[1] if len(mats) > 1 else None)
    return R, M


# ---------------------------------------------------------------------------------------------- matching and counting (:264-326)
def match_results(R: np.ndarray):
    """culane_metric2's return (:79-93) for a frame: (row_ind, col_ind, ious); empty when either side has no lanes."""
    from scipy.optimize import linear_sum_assignment
    if R.shape[0] == 0 or R.shape[1] == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), R
    row_ind, col_ind = linear_sum_assignment(1 - R)
    return row_ind, col_ind, R


def persistent_lanes(M: np.ndarray, iou_threshold: float):
    """matching_lane_instance (:306-326): the pairs (anno at t, anno at t-1) of the optimal assignment with IoU > threshold."""
    from scipy.optimize import linear_sum_assignment
    row_ind, col_ind = linear_sum_assignment(1 - M)
    check = M[row_ind, col_ind] > iou_threshold
    return row_ind[check], col_ind[check]


def _matched_iou(result, anno_idx) -> float:
    row_ind, col_ind, ious = result
    hit = (row_ind == anno_idx).nonzero()[0]
    return float(ious[anno_idx, col_ind[hit[0]]]) if len(hit) else 0.0


def count_inter_frame(M: np.ndarray, result_t, result_prev, iou_threshold: float) -> Tuple[int, int, int]:
    """metric_per_inter_frame (:264-304) -> (Ns, Nj, Nm).  `result_*` are `match_results` of R_t and R_t-1.  The three-way
    test is the reference's, with strict > and <: an IoU exactly at the threshold falls through to Ns."""
    Ns = Nj = Nm = 0
    for cur, prev in zip(*persistent_lanes(M, iou_threshold)):
        iou1, iou2 = _matched_iou(result_t, cur), _matched_iou(result_prev, prev)
        if (iou1 > iou_threshold and iou2 < iou_threshold) or (iou1 < iou_threshold and iou2 > iou_threshold):
            Nj += 1
        elif iou1 < iou_threshold and iou2 < iou_threshold:
            Nm += 1
        else:
            Ns += 1
    return Ns, Nj, Nm


# ---------------------------------------------------------------------------------------------- videos (:170-262)
def evaluate_frames(frames: Sequence, height: int, width: int, lane_width: int = 30, iou_threshold: float = 0.5,
                    batch_frames: int = 64, device="cuda", num_t: int = 1, ious: Optional[Callable] = None) -> List[Tuple[int, int, int]]:
    """mainMetric (:227-262) for one video: frames = [(anno_lanes, pred_lanes), ...] -> [(Ns, Nj, Nm)] per inter-frame
    (len(frames) - 1 of them).  Frames go to the device in batches of at most `batch_frames`; the last frame's annotated lanes
    are carried into the next batch and drawn again there, so the result does not depend on `batch_frames`.  `ious` replaces
    `device_ious` (tests run the host logic on a numpy backend)."""
    if num_t != 1:
        raise ValueError("only num_t = 1 is built (every shipped options file sets it)")
    if batch_frames < 1:
        raise ValueError("batch_frames must be positive")
    if ious is None:
        ious = lambda s, g, h, w, lw: device_ious(s, g, h, w, lw, device)      # noqa: E731
    frames = list(frames)
    out, carry, prev_result = [], None, None
    for b in range(0, len(frames), batch_frames):
        batch = frames[b:b + batch_frames]
        R, M = frame_ious(batch, carry, height, width, lane_width, ious)
        for r, m in zip(R, M):
            result = match_results(r)
            if m is not None:
                out.append(count_inter_frame(m, result, prev_result, iou_threshold))
            prev_result = result
        carry = batch[-1][0]
    return out


def video_datalist(names: Sequence[str]) -> dict:
    """get_video_datalist (:170-178): names grouped by their directory, in list order."""
    videos = {}
    for name in names:
        videos.setdefault(os.path.dirname(name), []).append(name)
    return videos


def summarize(per_video: dict) -> dict:
    """:212-225: totals over the videos and the rates (NaN when nothing persisted)."""
    Ns = sum(ns for v in per_video.values() for ns, _, _ in v)
    Nj = sum(nj for v in per_video.values() for _, nj, _ in v)
    Nm = sum(nm for v in per_video.values() for _, _, nm in v)
    n = Ns + Nj + Nm
    Rs, Rj, Rm = (float(Ns) / n, float(Nj) / n, float(Nm) / n) if n else (float("nan"),) * 3
    return {"Ns": Ns, "Nj": Nj, "Nm": Nm, "Rs": Rs, "Rj": Rj, "Rm": Rm, "per_video": per_video}


def evaluate(anno_dir: str, pred_dir: str, names: Sequence[str], height: int, width: int, lane_width: int = 30,
             iou_threshold: float = 0.5, batch_frames: int = 64, device="cuda", num_t: int = 1,
             ious: Optional[Callable] = None) -> dict:
    """eval_predictions (:197-225): `names` are the entries of the data list (frame names without extension; the label files
    are os.path.join(dir, name + '.lines.txt') as in :236-237) -> dict(Ns, Nj, Nm, Rs, Rj, Rm, per_video = {video: [(Ns, Nj, Nm)]})."""
    per_video = {}
    for video, members in video_datalist(names).items():
        frames = [(load_lanes(os.path.join(anno_dir, m + ".lines.txt")), load_lanes(os.path.join(pred_dir, m + ".lines.txt")))
                  for m in members]
        per_video[video] = evaluate_frames(frames, height, width, lane_width, iou_threshold, batch_frames, device, num_t, ious)
    return summarize(per_video)


def result_block(results: dict, list_path: str) -> str:
    """The block measure_IoU prints (:186-193)."""
    header = "=" * 20 + "Results ({})".format(os.path.basename(list_path)) + "=" * 20
    lines = [header]
    for metric in ("Ns", "Nj", "Nm", "Rs", "Rj", "Rm"):
        value = results[metric]
        lines.append("{}: {:.4f}".format(metric, value) if isinstance(value, float) else "{}: {}".format(metric, value))
    lines.append("=" * len(header))
    return "\n".join(lines) + "\n"


def main(argv=None) -> int:
    import getopt
    opts, _ = getopt.getopt(sys.argv[1:] if argv is None else argv, "ha:d:l:r:c:w:t:o:b:")
    o = {"-w": "30", "-t": "0.5", "-b": "64"}
    o.update(dict(opts))
    if "-h" in o or not all(k in o for k in ("-a", "-d", "-l", "-r", "-c")):
        print(__doc__)
        return 0 if "-h" in o else 2
    if not os.path.exists(o["-l"]):
        print(f"Error: file {o['-l']} not exist!", file=sys.stderr)
        return 1
    with open(o["-l"]) as fh:
        names = [line.strip() for line in fh if line.strip()]
    res = evaluate(o["-a"], o["-d"], names, int(o["-r"]), int(o["-c"]), int(o["-w"]), float(o["-t"]), int(o["-b"]))
    block = result_block(res, o["-l"])
    sys.stdout.write(block)
    if "-o" in o:
        with open(o["-o"], "w") as fh:
            fh.write(block)
    return 0


if __name__ == "__main__":
    sys.exit(main())
