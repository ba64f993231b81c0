"""Validation F1 / mIoU as a by-product of inference (DESIGN.md "Validation F1"): the CULane-style evaluator of `culane.py`
without its file protocol.  The polylines `infer_points_device` / `stream.polylines` leave on the device and a packed table of
annotations go through five graph nodes - memset, phnet_lane_eval_segments (text round trip, spline, cv::line end points),
phnet_lane_raster, phnet_lane_iou_groups, phnet_lane_eval_count (Kuhn-Munkres, counters, totals) - and `compute()` copies the
totals to the host once per validation pass.  The numbers are those of `culane.evaluate` on the `.lines.txt` files
`generate_predV2` would have written: equal tp / fp / fn, bit-equal miou.

    meter = LaneF1Meter(1280, 1920, lane_width=30, threshold=0.5, size=(800, 1920), max_images=64, n_offsets=36, max_lanes=4)
    gt = [t.cuda(non_blocking=True) for t in pack_eval_lanes(annotations, meter.max_gt_lanes, meter.max_gt_points)]   # once
    for frames, gt_points, gt_count, gt_num in batches:
        _, _, _, polylines = model.infer_points_device(frames)
        meter.update(polylines, gt_points, gt_count, gt_num)            # no host synchronisation
    print(meter.compute())                                              # one device -> host copy
"""
from typing import Optional, Sequence

import numpy as np
import torch

from .. import hip_ops as K
from . import culane
from .generate_lane import CROP_TOP


def pack_eval_lanes(frames_of_lanes: Sequence, max_lanes: int, max_points: int):
    """Host helper: [image][lane] -> array-like [n, 2] in evaluator coordinates (`culane.read_lane_file` of the annotation file) ->
    (points f32 [F,max_lanes,max_points,2], count i32 [F,max_lanes], num i32 [F]), zero padded, in pinned memory where a device is
    present (copy with non_blocking=True, once: the tensors can stay on the device across epochs).  An image with more than
    max_lanes lanes or a lane with more than max_points points raises: nothing is truncated."""
    if not (1 <= max_lanes <= K.LANE_EVAL_MAX_LANES and 2 <= max_points <= K.LANE_EVAL_MAX_POINTS):
        raise ValueError(f"max_lanes = {max_lanes}, max_points = {max_points} outside 1 <= lanes <= {K.LANE_EVAL_MAX_LANES}, "
                         f"2 <= points <= {K.LANE_EVAL_MAX_POINTS}")
    f = len(frames_of_lanes)
    points = np.zeros((f, max_lanes, max_points, 2), np.float32)
    count = np.zeros((f, max_lanes), np.int32)
    num = np.zeros((f,), np.int32)
    for i, lanes in enumerate(frames_of_lanes):
        if len(lanes) > max_lanes:
            raise ValueError(f"image {i} has {len(lanes)} lanes, max_lanes = {max_lanes}")
        num[i] = len(lanes)
        for l, lane in enumerate(lanes):
            pts = np.asarray(lane, dtype=np.float32).reshape(-1, 2) if len(lane) else np.zeros((0, 2), np.float32)
            if len(pts) > max_points:
                raise ValueError(f"lane {l} of image {i} has {len(pts)} points, max_points = {max_points}")
            count[i, l] = len(pts)
            points[i, l, :len(pts)] = pts
    tensors = tuple(torch.from_numpy(a) for a in (points, count, num))
    return tuple(x.pin_memory() for x in tensors) if torch.cuda.is_available() else tensors


class LaneF1Meter:
    """Accumulates the evaluator's tp / fp / fn / IoU sum on the device, per video row.  All buffers (segment table, masks, the
    static groups table, IoU matrices, per-image rows, totals) are allocated here once, so `update` is hipGraph-capturable and a
    replay reads and writes the same addresses.  mode "wire": the predictions are normalised polylines and go through the
    `.lines.txt` round trip with size = (H_crop, W_org) and crop_top; "raw": they are evaluator coordinates already."""

    def __init__(self, height: int, width: int, lane_width: int = 30, threshold: float = 0.5, size=(800, 1920),
                 crop_top: float = CROP_TOP, max_images: int = 64, max_gt_lanes: int = 8, max_gt_points: int = 64, max_lanes: int = 4,
                 n_offsets: int = 36, videos: int = 1, mode: str = "wire", device="cuda"):
        if lane_width < 1:
            raise ValueError("width_lane must be positive")                          # evaluate.cpp:116-121
        if mode not in K.LANE_EVAL_MODES:
            raise ValueError(f"mode must be one of {sorted(K.LANE_EVAL_MODES)}, got {mode!r}")
        if not (1 <= max_gt_lanes <= K.LANE_EVAL_MAX_LANES and 1 <= max_lanes <= K.LANE_EVAL_MAX_LANES
                and 2 <= max_gt_points <= K.LANE_EVAL_MAX_POINTS and 2 <= n_offsets <= K.LANE_EVAL_MAX_POINTS):
            raise ValueError(f"max_gt_lanes = {max_gt_lanes}, max_lanes = {max_lanes}, max_gt_points = {max_gt_points}, n_offsets = "
                             f"{n_offsets} outside 1 <= lanes <= {K.LANE_EVAL_MAX_LANES}, 2 <= points <= {K.LANE_EVAL_MAX_POINTS}")
        if max_images < 1 or videos < 1 or not (1 <= height <= 4096 and 1 <= width <= 4096):
            raise ValueError("max_images and videos must be positive, height and width in 1..4096")
        self.height, self.width, self.lane_width, self.threshold = int(height), int(width), int(lane_width), float(threshold)
        self.size, self.crop_top, self.mode = (float(size[0]), float(size[1])), float(crop_top), mode
        self.max_images, self.videos = int(max_images), int(videos)
        self.max_gt_lanes, self.max_gt_points, self.max_lanes, self.n_offsets = int(max_gt_lanes), int(max_gt_points), int(max_lanes), int(n_offsets)
        g, l, f = self.max_gt_lanes, self.max_lanes, self.max_images
        self.rows_per_lane = K.lane_eval_rows(n_offsets, max_gt_points)
        if f * (g + l) * self.rows_per_lane >= 1 << 31:
            raise ValueError("max_images * (max_gt_lanes + max_lanes) * rows per lane must stay below 2^31")
        dev = self.device = torch.device(device)
        i32 = dict(dtype=torch.int32, device=dev)
        self._segs = torch.zeros((f * (g + l), self.rows_per_lane, 5), **i32)
        self._lane_pts = torch.zeros((f, g + l), **i32)
        self._masks = torch.zeros((f * (g + l), self.height, (self.width + 31) // 32), **i32)
        table = [(i * (g + l), g, i * (g + l) + g, l, i * g * l) for i in range(f)]          # static: one group per image
        self._groups = torch.from_numpy(K.check_iou_groups(np.asarray(table, np.int32), f * (g + l))[0]).to(dev)
        self._iou = torch.zeros((f, g, l), dtype=torch.float64, device=dev)
        self._rows = dict(tp=torch.zeros(f, **i32), fp=torch.zeros(f, **i32), fn=torch.zeros(f, **i32),
                          iou_im=torch.zeros(f, dtype=torch.float64, device=dev), anno_match=torch.full((f, g), -1, **i32))
        # totals i64 [V,4], iou_tot f64 [V] and overflow i32 in one 8-byte-element buffer: one memset to reset, one copy to read
        self._acc = torch.zeros(self.videos * 5 + 1, dtype=torch.int64, device=dev)
        self._totals = self._acc[:self.videos * 4].view(self.videos, 4)
        self._iou_tot = self._acc[self.videos * 4:self.videos * 5].view(torch.float64)
        self._overflow = self._acc[self.videos * 5:].view(torch.int32)[:1]
        self._last = 0

    def reset(self) -> None:
        """Zeroes the totals (one memset on the current stream).  The rows of the last update stay where they are."""
        self._acc.zero_()

    def update(self, polylines: dict, gt_points: torch.Tensor, gt_count: torch.Tensor, gt_num: torch.Tensor,
               video: Optional[torch.Tensor] = None) -> None:
        """polylines: the dict of `infer_points_device` / `stream.polylines` (points f32 [..,L,S,2], count i32 [..,L], lanes_num i32
        [..]) with any leading shape of F <= max_images frames; gt_points f32 [F,G,P,2], gt_count i32 [F,G], gt_num i32 [F] (any
        leading shape of the same F frames) as `pack_eval_lanes` builds them; video i32 [F]: the accumulator row of each frame (row 0
        without it).  Memset, segments, raster, IoU and count on the current stream: no host synchronisation, nothing allocated."""
        g, l, s, p = self.max_gt_lanes, self.max_lanes, self.n_offsets, self.max_gt_points
        points, count, lanes_num = polylines["points"], polylines["count"], polylines["lanes_num"]
        if tuple(points.shape[-3:]) != (l, s, 2) or tuple(gt_points.shape[-3:]) != (g, p, 2):
            raise ValueError(f"LaneF1Meter.update: points [..,{l},{s},2] and gt_points [..,{g},{p},2] expected, got "
                             f"{tuple(points.shape)} and {tuple(gt_points.shape)}")
        f = lanes_num.numel()
        if not 1 <= f <= self.max_images or gt_num.numel() != f:
            raise ValueError(f"LaneF1Meter.update: {f} frames against {gt_num.numel()} annotated ones, max_images = {self.max_images}")
        if video is not None:
            video = video.reshape(f)
        n = f * (g + l)
        masks = self._masks[:n]
        masks.zero_()
        seg = K.lane_eval_segments(points.reshape(f, l, s, 2), count.reshape(f, l), lanes_num.reshape(f), gt_points.reshape(f, g, p, 2),
                                   gt_count.reshape(f, g), gt_num.reshape(f), self.mode, self.size, self.crop_top,
                                   out=dict(segs=self._segs[:n], lane_pts=self._lane_pts[:f]))
        K.lane_raster(seg["segs"].view(-1, 5), n, self.height, self.width, self.lane_width, masks=masks)
        K.lane_iou_groups_device(masks, self._groups[:f], f * g * l, self.width, self._iou[:f])
        K.lane_eval_count(self._iou[:f], seg["lane_pts"], g, self.threshold, self._totals, self._iou_tot, self._overflow, video=video,
                          out={k: v[:f] for k, v in self._rows.items()})
        self._last = f

    def per_image(self) -> dict:
        """The rows of the last update on the host: tp, fp, fn int32 [F], iou_im float64 [F], anno_match int32 [F,G] (the prediction
        index of each annotation, -1 = none), lane_pts int32 [F,G+L] (-1 = not in the evaluator's list, else the lane's points) and
        iou float64 [F,G,L], the lane IoU matrices (an entry of a lane that is not drawn is NaN)."""
        f = self._last
        out = {k: v[:f].cpu().numpy() for k, v in self._rows.items()}
        out["lane_pts"] = self._lane_pts[:f].cpu().numpy()
        out["iou"] = self._iou[:f].cpu().numpy()
        return out

    def iou_sum(self) -> float:
        """The evaluator's running IoU sum (row 0; one device -> host copy)."""
        return float(self._iou_tot[:1].cpu().numpy()[0])

    def compute(self) -> dict:
        """One device -> host copy -> the dict of `culane.summarize` over everything since the last reset (+ "images" and
        "overflow": images that reached the relabelling cap of phnet_lane_eval_count, 0 on any real input).  videos > 1: also
        "per_video", the summarize dict of every row, and "aggregate", `culane.aggregate` over the rows."""
        acc = self._acc.cpu().numpy()
        v = self.videos
        totals, iou_tot = acc[:v * 4].reshape(v, 4), acc[v * 4:v * 5].view(np.float64)
        overflow = int(acc[v * 5:].view(np.int32)[0])
        iou = 0.0
        for x in iou_tot.tolist():                                       # one row: the kernel's sum itself, bit for bit
            iou = x if v == 1 else iou + x
        tp, fp, fn, images = (int(x) for x in totals.sum(axis=0))
        res = culane.summarize(tp, fp, fn, iou, images)
        res.update(images=images, overflow=overflow)
        if v > 1:
            rows = [culane.summarize(int(r[0]), int(r[1]), int(r[2]), float(x), int(r[3])) for r, x in zip(totals, iou_tot)]
            res["per_video"] = rows
            g = lambda val: "nan" if val != val else "%g" % val             # what read_helper finds in an output file
            try:
                res["aggregate"] = culane.aggregate({i: dict(tp=str(r["tp"]), fp=str(r["fp"]), fn=str(r["fn"]), miou=g(r["miou"]))
                                                     for i, r in enumerate(rows)})
            except ZeroDivisionError:                                       # no true positive anywhere: the reference's script raises
                res["aggregate"] = None
        return res
