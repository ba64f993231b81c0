"""Host side of the device-resident lane polylines (csrc/lane_points.hip, hip_ops.lane_points).

`to_host` is the fast counterpart of `lanes_from_device` / `DetNetV2.predictions_to_pred`: the points already exist on the
device, so the host only copies and slices - no `.item()`, no per-lane torch / numpy arithmetic, no spline.  The evaluation
writers (evaluation/generate_lane.py: `format_pred_lines`, `generate_predV2`) read `.points` only and take `Polyline` objects as
they are; `Polyline.as_lane()` builds the reference-compatible `Lane` (with its scipy spline) for the callers that resample.

    rows, num, anchors, pl = model.infer_points_device(frames)            # or stream.step(frames); stream.polylines
    lines = to_host(pl["points"], pl["count"], pl["lanes_num"], pl["slot"], rows)
    lines[t][k].points                                                    # float64 [n,2], normalised (x, y)
"""
from typing import Dict, List, Optional

import numpy as np
import torch

from .libs.utils.lane import Lane


class Polyline:
    """One detected lane: `points` float64 [n,2] normalised (x, y) in the order of the host path (bottom of the image last),
    `metadata` with the keys of `Lane.metadata` (start_x, start_y, conf; numpy float32 scalars)."""
    __slots__ = ("points", "metadata")

    def __init__(self, points: np.ndarray, metadata: Dict):
        self.points = points
        self.metadata = metadata

    def as_lane(self) -> Lane:
        """The reference-compatible Lane (interpolating spline x(y), `to_array`), built on demand."""
        return Lane(points=self.points, metadata=dict(self.metadata))

    def __len__(self) -> int:
        return len(self.points)

    def __iter__(self):
        return iter(self.points)

    def __repr__(self) -> str:
        return f"[Polyline]\n{self.points}\n[/Polyline]"


def to_host(points: torch.Tensor, count: torch.Tensor, lanes_num: torch.Tensor, slot: torch.Tensor, kept_rows: torch.Tensor,
            track_id: Optional[torch.Tensor] = None) -> List:
    """points f32 [..,L,S,2], count i32 [..,L], lanes_num i32 [..], slot i32 [..,L] (hip_ops.lane_points) and the kept_rows
    [..,L,6+S] they were made from -> nested lists over the leading dimensions (streams; frames of a clip; clips x frames), the
    innermost a list of Polyline per frame.  No leading dimension: the Polyline list of the one frame.  track_id int32 [..,L]
    (hip_ops.lane_track: the id of each kept_rows slot): each Polyline's metadata gains "track_id", a Python int, taken through
    `slot` like the other keys; it travels in the same packed buffer.

    ONE device -> host transfer: the five tensors are PACKED on the device into one byte buffer (a single `torch.cat` launch of
    their byte views) and that buffer is copied once - five small copies would pay the copy latency five times, and a pinned
    staging area would have to be sized and owned per caller.  Everything after the copy is numpy slicing of that buffer."""
    lead = tuple(lanes_num.shape)
    L, S = points.shape[-3], points.shape[-2]
    if (tuple(points.shape) != lead + (L, S, 2) or tuple(count.shape) != lead + (L,) or tuple(slot.shape) != lead + (L,)
            or tuple(kept_rows.shape) != lead + (L, 6 + S)):
        raise ValueError(f"to_host: points {tuple(points.shape)} / count {tuple(count.shape)} / lanes_num {lead} / "
                         f"slot {tuple(slot.shape)} / kept_rows {tuple(kept_rows.shape)} do not belong together")
    if (points.dtype, kept_rows.dtype) != (torch.float32, torch.float32) or any(t.dtype != torch.int32 for t in (count, lanes_num, slot)):
        raise ValueError("to_host: f32 points / kept_rows and int32 count / lanes_num / slot expected")
    if track_id is not None and (tuple(track_id.shape) != lead + (L,) or track_id.dtype != torch.int32):
        raise ValueError(f"to_host: track_id must be int32 {lead + (L,)}, got {track_id.dtype} {tuple(track_id.shape)}")
    parts = (points, kept_rows, count, lanes_num, slot) + (() if track_id is None else (track_id,))      # all 4-byte elements: one int32 buffer
    packed = torch.cat([t.detach().contiguous().view(torch.int32).reshape(-1) for t in parts]).cpu().numpy()
    views, at = [], 0
    for t in parts:
        views.append(packed[at:at + t.numel()])
        at += t.numel()
    F = int(np.prod(lead, dtype=np.int64)) if lead else 1
    pts = views[0].view(np.float32).reshape(F, L, S, 2).astype(np.float64)     # exact widening, once for all lanes
    meta = views[1].view(np.float32).reshape(F, L, 6 + S)[:, :, 1:4]            # conf, start_y, start_x
    cnt, num, src = views[2].reshape(F, L), views[3].reshape(F), views[4].reshape(F, L)
    frames = [[Polyline(pts[f, k, :cnt[f, k]], {"start_x": meta[f, src[f, k], 2], "start_y": meta[f, src[f, k], 1],
                                               "conf": meta[f, src[f, k], 0]})
               for k in range(num[f])] for f in range(F)]
    if track_id is not None:
        ids = views[5].reshape(F, L)
        for f in range(F):
            for k, line in enumerate(frames[f]):
                line.metadata["track_id"] = int(ids[f, src[f, k]])
    for n in reversed(lead[1:]):                                                # nest like the leading dimensions
        frames = [frames[i:i + n] for i in range(0, len(frames), n)]
    return frames if lead else frames[0]
