"""Mask-level video metrics, the DAVIS pair: region similarity J and boundary F-measure F of a predicted and an annotated lane
mask per frame - the protocol of evaluation/evaluate_vid.py with video_metrics/jaccard.py and video_metrics/f_boundary.py, with
the pixel work on the GPU.

    python -m phnet_amd.evaluation.video -a ANNO_DIR -d PRED_DIR -l LIST -r HEIGHT -c WIDTH -w LANE_WIDTH [-b BATCH_FRAMES] [-o OUT]

Per frame the reference turns both masks into boundary maps (seg2bmap), dilates each by a disk of ceil(0.008 * diagonal) pixels
(skimage) and counts; that is seconds per full-size frame pair on the host.  Here one call (`phnet_mask_metrics`,
csrc/mask_metrics.hip) reduces a batch of mask pairs to seven integers per frame - three areas, two boundary sizes, two match
counts; the rules are numbered in include/phnet_hip.h and DESIGN.md "Mask metrics" - and J and F are float64 host arithmetic on
those integers, operation for operation what the reference does.  `device_counts` is the only device step and has no CPU
fallback: without the HIP library it raises; everything downstream takes the counts and runs anywhere.

The masks come from the device: `LaneRenderer.render(pl)["label_map"]` against a rendered annotation (`VideoMaskEval.update`), or,
on the command line, the `.lines.txt` pairs the other two evaluators read, drawn by the project's rasterisation rule
(`phnet_lane_raster`: straight segments between the truncated points, as the reference's mask writer draws them, testOL.py:165-227)
into one mask per frame and side.  No image files are read: the reference scores PNG files (skimage.io.imread), and no
image-reading library is available to test that against, so it is not built.

The boundary rule, the radius rule, the precision / recall / F branches and J are pinned to the reference's executed code
(tests/golden/video_metrics_tiny.json); the dilation is pinned to scipy.ndimage.binary_dilation with the same disk - PARITY
UNPINNED against skimage, which is not installed.  `t_stability.py` of the same directory is not built (evaluate_vid.py does not
call it).
"""
import json
import math
import os
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np

COUNTS = ("area_pred", "area_gt", "area_both", "n_fg", "n_gt", "fg_match", "gt_match")
WINDOW = 480                           # AverageMeter's deque(maxlen=480), evaluate_vid.py:19


def boundary_radius(h: int, w: int, bound_th: float = 0.008) -> int:
    """f_boundary.py:31-32 in float64: bound_th itself when bound_th >= 1, else ceil(bound_th * sqrt(h^2 + w^2)).  A fractional
    bound_th >= 1 raises: skimage's disk of a fractional radius is not a disk of that radius."""
    bound_th = float(bound_th)
    if not bound_th >= 0.0 or math.isinf(bound_th):
        raise ValueError(f"bound_th must be finite and >= 0, got {bound_th}")
    if bound_th >= 1:
        if bound_th != math.floor(bound_th):
            raise ValueError(f"bound_th >= 1 is a radius in pixels and must be an integer, got {bound_th}")
        return int(bound_th)
    return int(math.ceil(bound_th * math.sqrt(float(int(h) * int(h) + int(w) * int(w)))))


def _host(counts) -> np.ndarray:
    if hasattr(counts, "detach"):
        counts = counts.detach().cpu().numpy()
    c = np.asarray(counts)
    if c.dtype.kind not in "iu" or c.ndim < 1 or c.shape[-1] != len(COUNTS):
        raise ValueError(f"counts must be integers [.., {len(COUNTS)}], got {c.dtype} {c.shape}")
    return c.astype(np.int64)


def boundary_f(counts) -> np.ndarray:
    """counts int [.., 7] -> F float64 [..]: the four branches of f_boundary.py:52-63 and F = 0 when precision + recall == 0
    (:66-69); 2 * precision * recall / (precision + recall) in that order of operations."""
    c = _host(counts)
    n_fg, n_gt = c[..., 3], c[..., 4]
    full = (n_fg > 0) & (n_gt > 0)
    precision = np.where(full, c[..., 5] / np.where(full, n_fg, 1).astype(np.float64), np.where(n_fg == 0, 1.0, 0.0))
    recall = np.where(full, c[..., 6] / np.where(full, n_gt, 1).astype(np.float64), np.where(n_gt == 0, 1.0, 0.0))
    total = precision + recall
    return np.where(total == 0, 0.0, 2 * precision * recall / np.where(total == 0, 1.0, total))


def jaccard(counts, hw: Sequence[int], two_class: bool = True) -> np.ndarray:
    """counts int [.., 7], hw = (H, W) of the masks -> J float64 [..].
    two_class=False: db_eval_iou(mask, gt) (jaccard.py:26-33) - 1 when both masks are empty, else both / union.
    two_class=True: what evaluate_vid.py:55-57 computes, db_eval_iou on the stacked pairs (~mask, mask) and (~gt, gt): the
    background counts as a second class, (both + (HW - union)) / (union + (HW - both)).
    The reference sums its denominator in float32 (np.sum(..., dtype=np.float32)); that is exact below 2^24, so for every picture
    with 2 H W < 2^24 (two_class) or H W < 2^24 the two agree to the bit.  Beyond that this is the exact quotient of the two
    integers, rounded once, and the reference is not."""
    c = _host(counts)
    pixels = int(hw[0]) * int(hw[1])
    both = c[..., 2]
    union = c[..., 0] + c[..., 1] - both
    if two_class:
        return (both + (pixels - union)) / (union + (pixels - both)).astype(np.float64)
    return np.where(union == 0, 1.0, both / np.where(union == 0, 1, union).astype(np.float64))


def device_counts(pred, gt, bound_th: float = 0.008):
    """THE device step: pred, gt u8 [.., H, W] on the device (a non-zero byte is foreground) -> int64 [.., 7] on the device, the
    counts of COUNTS per frame at the radius `boundary_radius(H, W, bound_th)`.  No synchronisation; `boundary_f` and `jaccard`
    copy it to the host."""
    from .. import hip_ops as K
    return K.mask_metric_counts(pred, gt, boundary_radius(pred.shape[-2], pred.shape[-1], bound_th))


def window_mean(values: Sequence[float], window: Optional[int] = WINDOW) -> float:
    """AverageMeter.avg (evaluate_vid.py:25-31): np.sum over the last `window` values / their number; None: all of them.  NaN for
    no values (the reference divides by zero there)."""
    vals = np.asarray(list(values), np.float64)
    if window is not None:
        vals = vals[-int(window):]
    return float(np.sum(vals) / len(vals)) if len(vals) else float("nan")


class VideoMaskEval:
    """measure_video (evaluate_vid.py:33-64): J and F per frame, their mean per video, the mean of those over the videos.
    window: the reference keeps every list in a deque(maxlen=480), so only the LAST 480 frames of a video (and the last 480
    videos) enter a mean - reproduced by default; window=None is the plain mean.  two_class: `jaccard`'s form (True is the
    reference's).  Frames and videos count in the order they are given."""

    def __init__(self, window: Optional[int] = WINDOW, bound_th: float = 0.008, two_class: bool = True):
        if window is not None and int(window) < 1:
            raise ValueError("window must be positive or None")
        self.window = None if window is None else int(window)
        self.bound_th, self.two_class = bound_th, bool(two_class)
        self._videos: Dict[str, List] = {}

    def update(self, video: str, pred, gt) -> None:
        """pred, gt: device label maps u8 [.., H, W] of frames of `video`, in order.  Enqueues the device step and keeps its
        result on the device; nothing is copied before `summary`."""
        self.update_counts(video, device_counts(pred, gt, self.bound_th), pred.shape[-2:])

    def update_counts(self, video: str, counts, hw: Sequence[int]) -> None:
        """The same from counts [.., 7] (a tensor or an integer array) of masks of hw = (H, W)."""
        self._videos.setdefault(video, []).append((counts, (int(hw[0]), int(hw[1]))))

    def frame_values(self, video: str):
        """(J [n], F [n]) float64 of the video's frames."""
        js, fs = [], []
        for counts, hw in self._videos[video]:
            c = _host(counts).reshape(-1, len(COUNTS))
            js.append(jaccard(c, hw, self.two_class))
            fs.append(boundary_f(c))
        return np.concatenate(js), np.concatenate(fs)

    def summary(self) -> dict:
        """dict(J, F, per_video = {video: dict(J, F, frames)})."""
        per_video = {}
        for video in self._videos:
            j, f = self.frame_values(video)
            per_video[video] = dict(J=window_mean(j, self.window), F=window_mean(f, self.window), frames=int(len(j)))
        return dict(J=window_mean([v["J"] for v in per_video.values()], self.window),
                    F=window_mean([v["F"] for v in per_video.values()], self.window), per_video=per_video)


# ---------------------------------------------------------------------------------------------- the command line
def frame_masks(frames: Sequence, height: int, width: int, lane_width: int, device="cuda"):
    """frames: [(anno_lanes, pred_lanes)], a lane a list of (x, y) points -> (pred, gt) u8 [n, H, W] on the device: every lane of a
    frame's side drawn into ONE mask by the rule of phnet_lane_raster, between the truncated points."""
    import torch
    from .. import hip_ops as K
    from .temporal import lane_segments
    rows = []
    for k, (anno, pred) in enumerate(frames):
        for side, lanes in ((0, pred), (1, anno)):
            for lane in lanes:
                s = lane_segments(np.asarray(lane, np.float64))
                rows.append(np.concatenate([s, np.full((len(s), 1), 2 * k + side, np.int32)], axis=1))
    segs = np.concatenate(rows, axis=0) if rows else np.zeros((0, 5), np.int32)
    dev = torch.device(device)
    words = K.lane_raster(torch.from_numpy(np.ascontiguousarray(segs, dtype=np.int32)).to(dev), 2 * len(frames), height, width, lane_width)
    bit = torch.arange(32, dtype=torch.int32, device=dev)
    masks = ((words.unsqueeze(-1) >> bit) & 1).to(torch.uint8).reshape(len(frames), 2, height, -1)[..., :width]
    return masks[:, 0].contiguous(), masks[:, 1].contiguous()


def evaluate(anno_dir: str, pred_dir: str, names: Sequence[str], height: int, width: int, lane_width: int, batch_frames: int = 32,
             bound_th: float = 0.008, window: Optional[int] = WINDOW, device="cuda") -> dict:
    """`names`: the entries of the data list (frame names without extension, grouped into videos by their directory; the label
    files are os.path.join(dir, name + '.lines.txt')) -> `VideoMaskEval.summary()`."""
    from .temporal import load_lanes, video_datalist
    if batch_frames < 1:
        raise ValueError("batch_frames must be positive")
    ev = VideoMaskEval(window=window, bound_th=bound_th)
    for video, members in video_datalist(names).items():
        for b in range(0, len(members), batch_frames):
            frames = [(load_lanes(os.path.join(anno_dir, m + ".lines.txt")), load_lanes(os.path.join(pred_dir, m + ".lines.txt")))
                      for m in members[b:b + batch_frames]]
            pred, gt = frame_masks(frames, height, width, lane_width, device)
            ev.update(video, pred, gt)
    return ev.summary()


def result_block(results: dict, list_path: str) -> str:
    header = "=" * 20 + "Results ({})".format(os.path.basename(list_path)) + "=" * 20
    lines = [header]
    for video, v in results["per_video"].items():
        lines.append("{}: J {:.4f} F {:.4f} ({} frames)".format(video, v["J"], v["F"], v["frames"]))
    lines.append("J: {:.4f}".format(results["J"]))
    lines.append("F: {:.4f}".format(results["F"]))
    lines.append("=" * len(header))
    return "\n".join(lines) + "\n"


def main(argv=None) -> int:
    import getopt
    opts, _ = getopt.getopt(sys.argv[1:] if argv is None else argv, "ha:d:l:r:c:w:o:b:")
    o = {"-b": "32"}
    o.update(dict(opts))
    if "-h" in o or not all(k in o for k in ("-a", "-d", "-l", "-r", "-c", "-w")):
        print(__doc__)
        return 0 if "-h" in o else 2
    if not os.path.exists(o["-l"]):
        print(f"Error: file {o['-l']} not exist!", file=sys.stderr)
        return 1
    with open(o["-l"]) as fh:
        names = [line.strip() for line in fh if line.strip()]
    res = evaluate(o["-a"], o["-d"], names, int(o["-r"]), int(o["-c"]), int(o["-w"]), int(o["-b"]))
    sys.stdout.write(result_block(res, o["-l"]))
    if "-o" in o:
        with open(o["-o"], "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
