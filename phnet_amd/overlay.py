"""Lanes back on a picture, on the device (csrc/lane_draw.hip, hip_ops.lane_draw): label maps and camera-frame overlays from the
device-resident polylines, one launch for any number of frames.

Replaces the host drawing of the reference's test loop (testOL.py:165-227: `predlanesV2` / `generate_seg_from_line` map every
point with int(), draw with cv2.line lane by lane; libs/utils/utility.py:66-68 blends with the input).  The rules - point to
pixel, coverage, order, value, blend - are numbered in include/phnet_hip.h and DESIGN.md "Lane overlay".  The pixel shape is the
project's exact integer rule for a thick segment (oracle/culane_cpu.py raster_lane), so a map agrees with what the evaluator
counts; PARITY UNPINNED against cv2.line's scan conversion.  No CPU path.

A clip (frames of the network input; the reference's geometry: 1280 x 1920 frames, the top 480 rows cropped):

    rows, num, anchors, pl = model.infer_points_device(frames)            # [T,...] or [B,T,...]
    r = LaneRenderer((1280, 1920), sx=1920, sy=1280 - 480, oy=480, lane_width=12)
    seg = r.render(pl)["label_map"]                                       # u8 [T,1280,1920] (or [B,T,1280,1920]): 0 = background, k + 1 = lane k

A live camera, the lanes on the frame itself, one colour per track, inside the captured step:

    pre = ClipPreprocessor(320, 800, pixel_format="nv12", pitch=2048)
    r = LaneRenderer.for_preprocessor(pre, overlay=True, label_map=False, alpha=128)
    s = model.open_stream(frame_hw=(320, 800), raw=pre, polylines=True, track=True, render=r)
    s.step(surfaces)
    s.rendered["overlay"]                                                 # u8 [B,1280,1920,3], rewritten by every step
"""
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import hip_ops as K


def default_palette() -> np.ndarray:
    """u8 [256,3] RGB.  Entry 0 (background) is black.  Entry v >= 1 is the fully saturated colour at position
    h = ((v - 1) * 587) mod 1530 of the 1530-step hue wheel (sector i = h // 255, f = h % 255: (255, f, 0), (255 - f, 255, 0),
    (0, 255, f), (0, 255 - f, 255), (f, 0, 255), (255, 0, 255 - f) for i = 0 .. 5).  587 is prime and 587 / 1530 is close to the
    golden-ratio step, so the 255 entries are distinct and neighbouring values are far apart on the wheel."""
    pal = np.zeros((256, 3), dtype=np.uint8)
    for v in range(1, 256):
        i, f = divmod(((v - 1) * 587) % 1530, 255)
        pal[v] = ((255, f, 0), (255 - f, 255, 0), (0, 255, f), (0, 255 - f, 255), (f, 0, 255), (255, 0, 255 - f))[i]
    return pal


class LaneRenderer:
    """out_hw = (H, W) of the picture; sx, sy, oy: pixel = (trunc(x * sx), trunc(y * sy + oy)) of a normalised point (rule 1;
    sx = src_w, sy = src_h - crop, oy = crop is the reference's mapping).  lane_width 1..256 in pixels; alpha 0..256 (256: the lane
    colour replaces the pixel, 128: the 50/50 blend); palette u8 [256,3] (default_palette()).  label_map / overlay choose the outputs.
    The frames an overlay is drawn on (`render(frames=...)`) are u8 [.., *frame_shape]: src_format "rgb" (packed, [H,W,3]), "nv12"
    ([surface_rows*3//2, pitch]) or "yuyv" ([H, pitch]) with pitch / surface_rows / csc (yuv_matrix) as ClipPreprocessor defines
    them; `for_preprocessor` fills all of that in."""

    def __init__(self, out_hw: Sequence[int], sx: float, sy: float, oy: float, lane_width: int = 12, alpha: int = 256, palette=None,
                 label_map: bool = True, overlay: bool = False, device="cuda", src_format: str = "rgb", pitch: Optional[int] = None,
                 surface_rows: Optional[int] = None, csc=None):
        self.out_h, self.out_w = int(out_hw[0]), int(out_hw[1])
        self.sx, self.sy, self.oy = float(sx), float(sy), float(oy)
        self.lane_width, self.alpha = int(lane_width), int(alpha)
        self.label_map, self.overlay = bool(label_map), bool(overlay)
        if not (1 <= self.out_h <= K.LANE_DRAW_MAX_SIZE and 1 <= self.out_w <= K.LANE_DRAW_MAX_SIZE):
            raise ValueError(f"out_hw {self.out_h}x{self.out_w}: each side must be in [1, {K.LANE_DRAW_MAX_SIZE}]")
        if not 1 <= self.lane_width <= K.LANE_DRAW_MAX_WIDTH or not 0 <= self.alpha <= 256:
            raise ValueError(f"lane_width in [1, {K.LANE_DRAW_MAX_WIDTH}] and alpha in [0, 256] expected")
        if not all(np.isfinite(v) for v in (self.sx, self.sy, self.oy)):
            raise ValueError("sx, sy, oy must be finite")
        if not (self.label_map or self.overlay):
            raise ValueError("LaneRenderer: label_map and / or overlay")
        pal = default_palette() if palette is None else np.asarray(palette)
        if pal.shape != (256, 3) or pal.dtype != np.uint8:
            raise ValueError("palette must be uint8 [256,3]")
        self.palette = pal.copy()
        self.device = torch.device(device)
        self._palette_dev: Dict[torch.device, torch.Tensor] = {}
        if src_format not in ("rgb", "nv12", "yuyv"):
            raise ValueError(f"src_format must be 'rgb', 'nv12' or 'yuyv', got {src_format!r}")
        self.src_format = src_format
        h, w = self.out_h, self.out_w
        if src_format == "rgb":
            if pitch is not None or surface_rows is not None or csc is not None:
                raise ValueError("pitch / surface_rows / csc describe nv12 / yuyv surfaces; rgb frames are packed")
            self.pitch, self.chroma_offset, self.csc, self.frame_shape = 3 * w, 0, None, (h, w, 3)
        else:
            if w % 2 or (src_format == "nv12" and h % 2):
                raise ValueError(f"{src_format} frames of {h}x{w}: chroma is subsampled, the size must be even")
            if csc is None or len(csc) != 10:
                raise ValueError("nv12 / yuyv frames need csc, the 10 integers of yuv_matrix")
            row_bytes = w if src_format == "nv12" else 2 * w
            self.pitch = row_bytes if pitch is None else int(pitch)
            rows = h if surface_rows is None else int(surface_rows)
            if self.pitch < row_bytes or rows < h or (src_format == "nv12" and rows % 2) or (src_format == "yuyv" and rows != h):
                raise ValueError(f"pitch {self.pitch} / surface_rows {rows} do not hold {src_format} frames of {h}x{w}")
            self.csc = [int(v) for v in csc]
            self.chroma_offset = rows * self.pitch if src_format == "nv12" else 0
            self.frame_shape = (rows * 3 // 2, self.pitch) if src_format == "nv12" else (h, self.pitch)

    @classmethod
    def for_preprocessor(cls, pre, lane_width: int = 12, alpha: int = 256, palette=None, label_map: bool = True, overlay: bool = False):
        """The renderer of a ClipPreprocessor's camera: the picture has the camera's resolution (src_h x src_w, the rows above the
        crop included), points map the way the reference maps them (sx = src_w, sy = src_h - crop, oy = crop), and `frames` are what
        the pre-processor takes - same pixel format, pitch, surface rows and colour matrix."""
        yuv = pre.pixel_format != "rgb"
        return cls((pre.src_h, pre.src_w), sx=pre.src_w, sy=pre.src_h - pre.crop, oy=pre.crop, lane_width=lane_width, alpha=alpha,
                   palette=palette, label_map=label_map, overlay=overlay, device=pre.xi.device, src_format=pre.pixel_format,
                   pitch=pre.pitch if yuv else None, surface_rows=pre.surface_rows if yuv else None,
                   csc=list(pre._csc) if yuv else None)

    def prepare(self, device) -> torch.Tensor:
        """The palette on `device` (copied there once: call it before capturing `render` in a graph)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._palette_dev:
            self._palette_dev[device] = torch.from_numpy(self.palette).to(device)
        return self._palette_dev[device]

    def buffers(self, lead: Sequence[int], device=None) -> Dict[str, Optional[torch.Tensor]]:
        """Zeroed output tensors for frames with the leading dimensions `lead` (on the renderer's device unless one is named):
        what `render(out=...)` takes."""
        lead, device = tuple(int(v) for v in lead), self.device if device is None else device
        return dict(label_map=torch.zeros(lead + (self.out_h, self.out_w), dtype=torch.uint8, device=device) if self.label_map else None,
                    overlay=torch.zeros(lead + (self.out_h, self.out_w, 3), dtype=torch.uint8, device=device) if self.overlay else None)

    def render(self, polylines: Dict[str, torch.Tensor], frames: Optional[torch.Tensor] = None,
               tracks: Optional[Dict[str, torch.Tensor]] = None, out: Optional[Dict[str, torch.Tensor]] = None):
        """polylines: the dict of hip_ops.lane_points (points [..,L,S,2], count [..,L], lanes_num [..], slot [..,L]) with any
        leading dimensions (streams; frames of a clip; clips x frames).  frames: u8 [.., *frame_shape], the pictures under the overlay
        (None: black; ignored without overlay=True).  tracks: the dict of hip_ops.lane_track - lanes are then coloured by
        track_id (rule 4) instead of by their index.  out: dict(label_map=, overlay=) of caller-owned tensors (`buffers`).
        -> dict(label_map u8 [..,H,W] or None, overlay u8 [..,H,W,3] or None) on the device; one launch, no synchronisation."""
        pts, cnt, num = polylines["points"], polylines["count"], polylines["lanes_num"]
        if not (pts.is_cuda and cnt.is_cuda and num.is_cuda):
            raise RuntimeError("LaneRenderer.render: the polylines must be CUDA(HIP) tensors; phnet_amd has no CPU path")
        lead = tuple(num.shape)
        if pts.dim() != len(lead) + 3 or tuple(pts.shape[:len(lead)]) != lead or tuple(cnt.shape) != lead + (pts.shape[-3],):
            raise ValueError(f"render: points {tuple(pts.shape)} / count {tuple(cnt.shape)} / lanes_num {lead} do not belong together")
        L, S = pts.shape[-3], pts.shape[-2]
        dev = pts.device
        slot = track_id = None
        if tracks is not None:
            slot, track_id = polylines["slot"].reshape(-1, L), tracks["track_id"].reshape(-1, L)
        src = None
        if self.overlay and frames is not None:
            if tuple(frames.shape) != lead + self.frame_shape:
                raise ValueError(f"render: frames {tuple(frames.shape)}, expected {lead + self.frame_shape} ({self.src_format})")
            src = frames.reshape(-1, *self.frame_shape)
        flat = {}
        for name, want, tail in (("label_map", self.label_map, (self.out_h, self.out_w)), ("overlay", self.overlay, (self.out_h, self.out_w, 3))):
            if not want:
                flat[name] = False
            elif out is None or out.get(name) is None:
                flat[name] = True
            else:
                if tuple(out[name].shape) != lead + tail or not out[name].is_contiguous():
                    raise ValueError(f"render: out[{name!r}] must be contiguous {lead + tail}, got {tuple(out[name].shape)}")
                flat[name] = out[name].reshape((-1,) + tail)
        got = K.lane_draw(pts.reshape(-1, L, S, 2), cnt.reshape(-1, L), num.reshape(-1), (self.out_h, self.out_w), self.sx, self.sy,
                          self.oy, self.lane_width, slot=slot, track_id=track_id, src=src,
                          src_format="none" if src is None else self.src_format, pitch=self.pitch, chroma_offset=self.chroma_offset,
                          csc=self.csc, palette=self.prepare(dev) if self.overlay else None, alpha=self.alpha,
                          label_map=flat["label_map"], overlay=flat["overlay"])
        return {k: None if v is None else v.reshape(lead + tuple(v.shape[1:])) for k, v in got.items()}
