"""Lane identities across frames (csrc/lane_track.hip, hip_ops.lane_track): the device state of the tracker and the defaults
the model layers share.

The detector's per-frame result is an unordered set of up to `max_lanes` kept rows in NMS order.  `phnet_lane_track` gives every
kept row a `track_id` that stays with the lane from frame to frame (rules: include/phnet_hip.h, DESIGN.md "Lane identities"),
without the result leaving the device:

    s = model.open_stream(streams=B, frame_hw=(H, W), track=True)      # the launch follows the decode inside the captured step
    rows, num, anchors = s.step(frames)
    s.tracks["track_id"], s.tracks["hits"]                             # int32 [B,max_lanes]: -1 / 0 where there is no lane
    track_id, hits = model.track_clips(rows, num)                      # clips: [T,..] or [B,T,..] results, fresh state, one launch
"""
from typing import Optional, Tuple

import numpy as np
import torch


class TrackState:
    """Tracker state of B streams with M = max_tracks slots each, allocated once: id int32 [B,M] (0 = free slot), missed
    int32 [B,M] (frames since the slot's last match), hits int32 [B,M] (frames it matched, the birth included), ext int32
    [B,M,2] (start, end offset index of the last matched row), x f32 [B,M,S] (that row's xs, copied) and next_id int32 [B] (the
    id the stream's next new lane gets; starts at 1)."""

    def __init__(self, streams: int, max_tracks: int, n_offsets: int, device):
        B, M, S = int(streams), int(max_tracks), int(n_offsets)
        if B < 1 or not 1 <= M <= 64 or not 2 <= S <= 256:
            raise ValueError("TrackState: streams >= 1, 1 <= max_tracks <= 64 and 2 <= n_offsets <= 256 expected")
        i32 = dict(dtype=torch.int32, device=device)
        self.id = torch.zeros((B, M), **i32)
        self.missed = torch.zeros((B, M), **i32)
        self.hits = torch.zeros((B, M), **i32)
        self.ext = torch.zeros((B, M, 2), **i32)
        self.x = torch.zeros((B, M, S), dtype=torch.float32, device=device)
        self.next_id = torch.ones((B,), **i32)

    def tensors(self) -> Tuple[torch.Tensor, ...]:
        """The six state tensors in the order of the C-ABI."""
        return self.id, self.missed, self.hits, self.ext, self.x, self.next_id

    def reset(self, mask: Optional[torch.Tensor] = None):
        """Free the slots of all streams, or of those where mask (bool [B], on the state's device) is set.  next_id is kept: ids
        never repeat within one TrackState, across camera cuts too.  Stream-ordered, outside any graph."""
        if mask is None:
            self.id.zero_()
        else:
            self.id.masked_fill_(mask.reshape(-1, 1), 0)


def track_defaults(model, max_tracks=None, max_age=None, match_thres=None) -> Tuple[int, int, float]:
    """(max_tracks, max_age, thr) for a RouterOL of either family.  max_tracks defaults to 2 * max_lanes.  max_age defaults to
    the model's save_freq_max - how long the network itself remembers a lane.  match_thres is in pixels of the network input like
    nms_thres and defaults to it (two rows closer than that within one frame are one lane by the model's own definition - a
    choice, not a tuned value); the kernel gets float32(match_thres / (img_w - 1)), the scale phnet_lane_decode applies to the xs
    before NMS."""
    det = model.head
    L = int(det.cfg.max_lanes)
    M = min(2 * L, 64) if max_tracks is None else int(max_tracks)
    age = int(model.save_freq_max) if max_age is None else int(max_age)
    px = float(det.cfg.test_parameters.nms_thres) if match_thres is None else float(match_thres)
    if not L <= M <= 64:
        raise ValueError(f"max_tracks must be in [max_lanes = {L}, 64], got {M}")
    if age < 0 or not (np.isfinite(px) and px > 0):
        raise ValueError("max_age >= 0 and a finite match_thres > 0 expected")
    return M, age, float(np.float32(px / (det.img_w - 1)))
