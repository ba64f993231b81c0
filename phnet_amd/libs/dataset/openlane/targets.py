"""Training targets on the GPU: annotated lane points -> the [max_lanes, 6+S] label rows that Criterion4OL and
GraphedTrainStep(frames, lanes) consume.

Replaces the label half of the reference's per-frame CPU pipeline (libs/dataset/openlane/datasetOL.py:47-59 crop / flip,
transforms.py:251-347 transform_annotation / filter_lane / sample_lane, which runs behind imgaug and scipy) with ONE launch for all
frames (csrc/lane_targets.hip); `ClipPreprocessor` is the image half.  No CPU path: the points must already be on the device
(`pack_annotations` pads Python / numpy annotation lists into pinned host tensors to copy from).

Arithmetic: the reference's float64 path, rule by rule (include/phnet_hip.h), with scipy's InterpolatedUnivariateSpline solved
explicitly (line, parabola, not-a-knot cubic spline).  Pinned to the reference's own executed code on tests/golden/targets_tiny.json.
PARITY UNPINNED (imgaug is not installed here): the arithmetic of its Resize on line strings - this module uses x * (out_w / src_w)
and y * (out_h / (src_h - crop)), each ratio formed once in double - and of clip_out_of_image_() (transforms.py:68), which `clip=True`
builds by the project's own rule 0c (include/phnet_hip.h): every lane is cut at the rectangle 0 <= x <= out_w - 1e-3,
0 <= y <= out_h - 1e-3, the crossing points are inserted, and a lane that leaves the image and comes back gives several fragments,
each a lane of its own with its own label row.  The 1e-3 inset is imgaug's, recalled from memory; imgaug's own point test is
x < out_w, so a sliver of 1e-3 px is treated differently here (DESIGN.md "Training targets").  With `augment=` (augment.py: rule 0b,
the flip and the affine of the augmented image applied to the points) more points leave the image, so clipping matters more there.
The constructor default clip=False keeps the rows of the unclipped entries.

The reference's retry loop (transforms.py:63-75) is not a missing piece: it retries only when transform_annotation raises, which no
input that the rules accept can make it do (DESIGN.md "Training augmentation").  In its place `frag_count=` gives the number of
surviving fragments per frame, on the device: a caller who wants to redraw a frame whose augmentation left no lane reads one integer."""
from typing import Optional, Sequence

import numpy as np
import torch

from phnet_amd import hip_ops as K


def sample_rows(img_h: int, num_points: int) -> np.ndarray:
    """cfg.offsets_ys of options4OL.py:146-148, exactly as numpy builds it: float64, bottom to top; its last entry is not exactly
    0 (-8.5e-13 for 320 / 35), so a lane whose top point has y == 0.0 does not get that row."""
    strip_size = img_h / (num_points - 1)
    ys = np.arange(img_h, -1, -strip_size)
    if len(ys) != num_points:
        raise ValueError(f"np.arange({img_h}, -1, -{img_h}/{num_points - 1}) has {len(ys)} entries, not num_points = {num_points}")
    return ys


class TargetEncoder:
    """cfg-like arguments as in options/options4OL.py (height, width, num_points, max_lanes; org 1280x1920, crop_size 480)."""

    def __init__(self, out_h: int, out_w: int, num_points: int, max_lanes: int, src_h: int = 1280, src_w: int = 1920,
                 crop_size: int = 480, device="cuda", clip: bool = False):
        self.clip = bool(clip)
        self.out_h, self.out_w, self.src_h, self.src_w, self.crop = int(out_h), int(out_w), int(src_h), int(src_w), int(crop_size)
        self.num_points, self.max_lanes = int(num_points), int(max_lanes)
        if not 0 <= self.crop < self.src_h:
            raise ValueError("crop_size must leave at least one row")
        if not (2 <= self.num_points <= K.LANE_TARGETS_MAX_OFFSETS and 1 <= self.max_lanes <= K.LANE_TARGETS_MAX_ROWS):
            raise ValueError(f"num_points = {num_points}, max_lanes = {max_lanes} outside 2 <= S <= 256, 1 <= R <= 64")
        self.strip_size = self.out_h / (self.num_points - 1)
        self.scale_x = float(self.out_w) / float(self.src_w)
        self.scale_y = float(self.out_h) / float(self.src_h - self.crop)
        self.offsets_ys = torch.from_numpy(sample_rows(self.out_h, self.num_points)).to(torch.device(device))

    @classmethod
    def for_preprocessor(cls, pre, num_points: int, max_lanes: int, clip: bool = False) -> "TargetEncoder":
        """The label half of a ClipPreprocessor: same output size, source size, crop and device."""
        return cls(pre.out_h, pre.out_w, num_points, max_lanes, src_h=pre.src_h, src_w=pre.src_w, crop_size=pre.crop, device=pre.xi.device,
                   clip=clip)

    def __call__(self, points: torch.Tensor, counts: torch.Tensor, lanes_num: torch.Tensor, flip: bool = False,
                 out: Optional[torch.Tensor] = None, augment=None, clip: Optional[bool] = None,
                 frag_count: Optional[torch.Tensor] = None) -> torch.Tensor:
        """points f32 [T,Lin,P,2] in source (camera) pixels, counts i32 [T,Lin], lanes_num i32 [T], all on the device (leading
        dimensions [B,T] are accepted) -> float32 [T,max_lanes,6+S].  flip: the clip was mirrored (datasetOL.py:54-55).
        out: a buffer of that shape to write into, e.g. the `lanes` of a GraphedTrainStep - then nothing is allocated and nothing
        waits for the device, so the call can be captured in a graph.
        augment: the AugmentParams (augment.py) of the same frames, on the device - the labels follow the augmented image
        (phnet_lane_targets_aug); None is the plain entry, exactly as without the argument.
        clip: rule 0c for this call (phnet_lane_targets_clip); None takes the constructor's.  Needs P <= 254.
        frag_count: an int32 [T] (or [B,T]) buffer on the device, written with the surviving fragments of each frame before the max_lanes
        cap (without clip: the surviving lanes) - 0 marks a frame whose augmentation left no lane."""
        clip = self.clip if clip is None else bool(clip)
        if not (points.is_cuda and counts.is_cuda and lanes_num.is_cuda):
            raise RuntimeError("TargetEncoder: CUDA(HIP) tensors expected; phnet_amd has no CPU path")
        if points.dim() < 4 or points.shape[-1] != 2:
            raise ValueError("TargetEncoder: points [..,Lin,P,2] expected")
        lead, (lin, p) = tuple(points.shape[:-3]), points.shape[-3:-1]
        if tuple(counts.shape) != lead + (lin,) or tuple(lanes_num.shape) != lead:
            raise ValueError(f"TargetEncoder: points {tuple(points.shape)} vs counts {tuple(counts.shape)}, lanes_num {tuple(lanes_num.shape)}")
        shape = lead + (self.max_lanes, 6 + self.num_points)
        if out is not None and tuple(out.shape) != shape:
            raise ValueError(f"TargetEncoder: out must be {shape}, got {tuple(out.shape)}")
        if frag_count is not None and (tuple(frag_count.shape) != lead or frag_count.dtype != torch.int32 or not frag_count.is_cuda):
            raise ValueError(f"TargetEncoder: frag_count must be int32 {lead} on the device")
        for t, name in ((points, "points"), (counts, "counts"), (lanes_num, "lanes_num"), (out, "out"), (frag_count, "frag_count")):
            if t is not None and not t.is_contiguous():
                raise RuntimeError(f"TargetEncoder: {name} must be contiguous")
        kw = dict(crop=self.crop, src_w=self.src_w, scale_x=self.scale_x, scale_y=self.scale_y, flip=flip,
                  out=None if out is None else out.view(-1, self.max_lanes, 6 + self.num_points))
        args = (points.view(-1, lin, p, 2), counts.view(-1, lin), lanes_num.view(-1), self.offsets_ys, self.max_lanes, self.out_h, self.out_w,
                self.strip_size)
        if augment is not None and (len(augment) != args[2].shape[0] or augment.device != points.device):
            raise ValueError(f"TargetEncoder: an AugmentParams of {args[2].shape[0]} frames on {points.device} expected")
        if clip or frag_count is not None:
            flat = K.lane_targets_clip(*args, None if augment is None else augment.flip2, None if augment is None else augment.fwd,
                                       clip=clip, frag_count=None if frag_count is None else frag_count.view(-1), **kw)
        elif augment is None:
            flat = K.lane_targets(*args, **kw)
        else:
            flat = K.lane_targets_aug(*args, augment.flip2, augment.fwd, **kw)
        return flat.view(shape) if out is None else out


def pack_annotations(frames_of_lanes: Sequence, max_in_lanes: int, max_points: int, clip: bool = False):
    """Host helper: [frame][lane] -> array-like [n, 2] of (x, y) -> (points f32 [T,max_in_lanes,max_points,2], counts i32
    [T,max_in_lanes], lanes_num i32 [T]), zero padded, in pinned memory where a device is present (copy with non_blocking=True).
    A frame with more than max_in_lanes lanes or a lane with more than max_points points raises: nothing is truncated.
    clip: the tensors are for an encoder with clip=True, which takes max_points <= 254."""
    if clip and max_points > K.LANE_TARGETS_MAX_POINTS_CLIP:
        raise ValueError(f"max_points = {max_points} outside 2 <= P <= 254 with clip")
    if not (1 <= max_in_lanes <= K.LANE_TARGETS_MAX_IN_LANES and 2 <= max_points <= K.LANE_TARGETS_MAX_POINTS):
        raise ValueError(f"max_in_lanes = {max_in_lanes}, max_points = {max_points} outside 1 <= Lin <= 64, 2 <= P <= 256")
    t = len(frames_of_lanes)
    points = np.zeros((t, max_in_lanes, max_points, 2), np.float32)
    counts = np.zeros((t, max_in_lanes), np.int32)
    lanes_num = np.zeros((t,), np.int32)
    for f, lanes in enumerate(frames_of_lanes):
        if len(lanes) > max_in_lanes:
            raise ValueError(f"frame {f} has {len(lanes)} lanes, max_in_lanes = {max_in_lanes}")
        lanes_num[f] = len(lanes)
        for l, lane in enumerate(lanes):
            pts = np.asarray(lane, dtype=np.float32).reshape(-1, 2) if len(lane) else np.zeros((0, 2), np.float32)
            if len(pts) > max_points:
                raise ValueError(f"lane {l} of frame {f} has {len(pts)} points, max_points = {max_points}")
            counts[f, l] = len(pts)
            points[f, l, :len(pts)] = pts
    pin = torch.cuda.is_available()
    tensors = tuple(torch.from_numpy(a) for a in (points, counts, lanes_num))
    return tuple(x.pin_memory() for x in tensors) if pin else tensors
