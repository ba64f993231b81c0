"""Clip pre-processing on the GPU: decoded uint8 frames (packed RGB, or the NV12 / YUYV surfaces decoders and cameras emit) -> the
normalised float clip the model consumes.

Replaces the image half of the reference's per-frame CPU pipeline (libs/dataset/openlane/datasetOL.py:40-52 crop / flip,
transforms.py:150-156 iaa.Resize = cv2 INTER_CUBIC on uint8, datasetOL.py:63-75 ToTensor + Normalize, :11-17 stacking) with ONE
launch per clip (csrc/preprocess.hip).  The label half (annotated points -> the [max_lanes, 6+S] target rows,
transforms.py:251-347) is `TargetEncoder` in targets.py beside this file; `TargetEncoder.for_preprocessor(pre, ...)` takes its
geometry from a ClipPreprocessor.  Training augmentation (augment.py beside this file) runs behind the resize: `__call__(...,
augment=params)`.  No CPU path: the frames must already be on the device.

Arithmetic: OpenCV's 8-bit bicubic resize as published (half-pixel centres, a = -0.75 kernel, 11-bit fixed-point taps that
sum to 2048, replicated borders, rounding 22-bit shift, saturation).  PARITY UNPINNED: cv2 / imgaug are not installed here
and the reference ships no image fixture; the kernel is held bit-exactly to a numpy restatement of the same algorithm
(oracle/preprocess_cpu.py)."""
import ctypes
from typing import Optional, Sequence

import numpy as np
import torch

from phnet_amd._lib import check, lib

_COEF_BITS = 11


def _axis_table(n_dst: int, n_src: int):
    """Clamped source indices [n_dst,4] int32 and fixed-point cubic taps [n_dst,4] int16 of one axis, as OpenCV's published
    imgproc/src/resize.cpp builds them for 8-bit INTER_CUBIC (the 4.x sources: cv::resize -> the generic path's coefficient
    loop + interpolateCubic): `fx = (float)((dx + 0.5) * scale - 0.5); sx = cvFloor(fx); fx -= sx;` - the source coordinate
    is ROUNDED TO FLOAT before its floor is taken and the fraction is a float subtraction - and every tap is stored as
    `saturate_cast<short>(c * 2048)` on its own: the four taps are NOT renormalised to sum to 2048 (they sum to 2047..2049)."""
    a = np.float32(-0.75)
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * (np.float64(n_src) / n_dst) - 0.5).astype(np.float32)
    s = np.floor(f)
    fx = (f - s).astype(np.float32)
    c0 = ((a * (fx + 1) - 5 * a) * (fx + 1) + 8 * a) * (fx + 1) - 4 * a
    c1 = ((a + 2) * fx - (a + 3)) * fx * fx + 1
    c2 = ((a + 2) * (1 - fx) - (a + 3)) * (1 - fx) * (1 - fx) + 1
    c3 = np.float32(1.0) - c0 - c1 - c2
    q = np.clip(np.rint(np.stack([c0, c1, c2, c3], axis=1).astype(np.float32) * np.float32(1 << _COEF_BITS)), -32768, 32767).astype(np.int32)
    idx = np.clip(s.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, n_src - 1).astype(np.int32)
    return idx, q.astype(np.int16)


_STANDARDS = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}      # (Kr, Kb) of ITU-R BT.601 / BT.709
_FORMATS = {"nv12": 0, "yuyv": 1}
_CSC_BITS = 20


def yuv_matrix(standard: str = "bt601", full_range: bool = False) -> np.ndarray:
    """int32 [10] for phnet_preprocess_yuv: y0, then the Y'CbCr -> R'G'B' matrix row-major (rows R, G, B; columns Y, U, V) as
    rint(coefficient * 2^20), derived in float64 from the standard's luma weights (Kr, Kb; Kg = 1 - Kr - Kb):
        R = sy (Y - y0)                                       + 2 (1 - Kr) sc (V - 128)
        G = sy (Y - y0) - 2 Kb (1 - Kb) / Kg sc (U - 128) - 2 Kr (1 - Kr) / Kg sc (V - 128)
        B = sy (Y - y0) + 2 (1 - Kb) sc (U - 128)
    limited ("video") range: y0 = 16, sy = 255/219, sc = 255/224; full range: y0 = 0, sy = sc = 1."""
    if standard not in _STANDARDS:
        raise ValueError(f"matrix must be one of {sorted(_STANDARDS)}, got {standard!r}")
    kr, kb = (np.float64(v) for v in _STANDARDS[standard])
    kg = 1.0 - kr - kb
    y0, sy, sc = (0, np.float64(1.0), np.float64(1.0)) if full_range else (16, np.float64(255.0) / 219.0, np.float64(255.0) / 224.0)
    m = np.array([[sy, 0.0, 2.0 * (1.0 - kr) * sc],
                  [sy, -2.0 * kb * (1.0 - kb) / kg * sc, -2.0 * kr * (1.0 - kr) / kg * sc],
                  [sy, 2.0 * (1.0 - kb) * sc, 0.0]], dtype=np.float64)
    return np.concatenate([[y0], np.rint(m * (1 << _CSC_BITS)).reshape(-1)]).astype(np.int32)


class ClipPreprocessor:
    """cfg-like arguments as in options/options4OL.py:101-108 (org 1280x1920, crop_size 480, mean / std of ImageNet).

    pixel_format: what the frames are.  "rgb" (default): packed 8-bit RGB [T,src_h,src_w,3].  "nv12": what video decoders emit - a
    surface of `pitch` bytes per row (default src_w) holding `surface_rows` luma rows (default src_h; even, >= src_h) and then
    surface_rows/2 rows of interleaved U,V: [T, surface_rows*3//2, pitch].  "yuyv": what USB / V4L2 cameras emit - packed 4:2:2 rows
    Y0 U Y1 V of `pitch` bytes (default 2*src_w): [T, src_h, pitch].  `frame_shape` is that per-frame shape.  matrix ("bt601" |
    "bt709") and full_range choose the colour matrix (`yuv_matrix`); chroma is replicated.  The conversion happens inside the one
    launch, tap by tap in integers, and the result equals this class in "rgb" form on the converted image bit for bit."""

    def __init__(self, out_h: int, out_w: int, src_h: int = 1280, src_w: int = 1920, crop_size: int = 480,
                 mean: Sequence[float] = (0.485, 0.456, 0.406), std: Sequence[float] = (0.229, 0.224, 0.225), device="cuda",
                 pixel_format: str = "rgb", pitch: Optional[int] = None, surface_rows: Optional[int] = None, matrix: str = "bt601",
                 full_range: bool = False):
        self.out_h, self.out_w, self.src_h, self.src_w, self.crop = int(out_h), int(out_w), int(src_h), int(src_w), int(crop_size)
        if not 0 <= self.crop < self.src_h:
            raise ValueError("crop_size must leave at least one row")
        self.pixel_format = pixel_format
        if pixel_format == "rgb":
            if pitch is not None or surface_rows is not None:
                raise ValueError("pitch / surface_rows describe nv12 / yuyv surfaces; rgb frames are packed")
            self.pitch = self.surface_rows = self._csc = None
        elif pixel_format in _FORMATS:
            if self.src_w % 2 or (pixel_format == "nv12" and self.src_h % 2):
                raise ValueError(f"{pixel_format} frames of {self.src_h}x{self.src_w}: chroma is subsampled, the size must be even")
            row_bytes = self.src_w if pixel_format == "nv12" else 2 * self.src_w
            self.pitch = row_bytes if pitch is None else int(pitch)
            if self.pitch < row_bytes:
                raise ValueError(f"pitch {self.pitch} < the {row_bytes} bytes of a {pixel_format} row of {self.src_w} pixels")
            self.surface_rows = self.src_h if surface_rows is None else int(surface_rows)
            if pixel_format == "nv12" and (self.surface_rows % 2 or self.surface_rows < self.src_h):
                raise ValueError(f"surface_rows {self.surface_rows}: an even number >= src_h {self.src_h} expected")
            if pixel_format == "yuyv" and self.surface_rows != self.src_h:
                raise ValueError("yuyv frames have src_h rows; surface_rows applies to nv12")
            csc = yuv_matrix(matrix, full_range)
            self._csc = (ctypes.c_int32 * 10)(*[int(v) for v in csc])
        else:
            raise ValueError(f"pixel_format must be 'rgb', 'nv12' or 'yuyv', got {pixel_format!r}")
        xi, xc = _axis_table(self.out_w, self.src_w)
        yi, yc = _axis_table(self.out_h, self.src_h - self.crop)
        dev = torch.device(device)
        self.xi, self.xc = torch.from_numpy(xi).to(dev), torch.from_numpy(xc).to(dev)
        self.yi, self.yc = torch.from_numpy(yi).to(dev), torch.from_numpy(yc).to(dev)
        self._mean = (ctypes.c_float * 3)(*[float(v) for v in mean])
        self._std = (ctypes.c_float * 3)(*[float(v) for v in std])
        self._stage, self._augmenter = {}, None                   # augment=: the resized 8-bit frames per (T, device); the ClipAugmenter

    @property
    def frame_shape(self):
        """Shape of ONE input frame: (src_h, src_w, 3) rgb, (surface_rows*3//2, pitch) nv12, (src_h, pitch) yuyv."""
        if self.pixel_format == "rgb":
            return (self.src_h, self.src_w, 3)
        if self.pixel_format == "nv12":
            return (self.surface_rows * 3 // 2, self.pitch)
        return (self.src_h, self.pitch)

    def __call__(self, frames_u8: torch.Tensor, flip: bool = False, layout: str = "nchw", return_u8: bool = False, augment=None,
                 out: Optional[torch.Tensor] = None):
        """frames_u8 [T, *frame_shape] uint8 on the device -> float32 [T,3,out_h,out_w] ("nchw", the reference's `img`) or
        [T,out_h,out_w,4] ("nhwc4", the stem's staging layout); with return_u8 also the resized 8-bit RGB frames.
        augment: an AugmentParams (augment.py) of T frames on the device - the resize launch writes the 8-bit frames into a staging
        buffer this object keeps per T, and the augment launch (phnet_augment_u8; with a stencil table in the params
        phnet_augment_stencil_u8, whose own staging buffer the ClipAugmenter keeps per T) turns them into the result (return_u8: the AUGMENTED
        8-bit frames); give the same table to TargetEncoder.  out: the float buffer to write into; with it (and, with augment, after one
        call of the same T) nothing is allocated, so the call can be captured in a graph."""
        if frames_u8.dim() != 1 + len(self.frame_shape) or tuple(frames_u8.shape[1:]) != self.frame_shape:
            raise ValueError(f"frames of {'x'.join(map(str, frames_u8.shape[1:]))}, built for {self.pixel_format} "
                             f"{'x'.join(map(str, self.frame_shape))}")
        if not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or not frames_u8.is_contiguous():
            raise RuntimeError(f"ClipPreprocessor: contiguous uint8 CUDA(HIP) frames [T,{','.join(map(str, self.frame_shape))}] expected; "
                               "phnet_amd has no CPU path")
        if layout not in ("nchw", "nhwc4"):
            raise ValueError("layout must be 'nchw' or 'nhwc4'")
        t, dev = frames_u8.shape[0], frames_u8.device
        shape = (t, 3, self.out_h, self.out_w) if layout == "nchw" else (t, self.out_h, self.out_w, 4)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
            raise ValueError(f"ClipPreprocessor: out must be contiguous float32 {shape} on {dev}")
        if augment is not None:
            stage = self._stage.get((t, dev))
            if stage is None:
                stage = self._stage[(t, dev)] = torch.empty((t, self.out_h, self.out_w, 3), dtype=torch.uint8, device=dev)
            u8 = stage
        else:
            u8 = torch.empty((t, self.out_h, self.out_w, 3), dtype=torch.uint8, device=dev) if return_u8 else None
        mean, std = ctypes.cast(self._mean, ctypes.c_void_p), ctypes.cast(self._std, ctypes.c_void_p)
        if self.pixel_format == "rgb":
            check(lib().phnet_preprocess_u8(frames_u8.data_ptr(), out.data_ptr(), None if u8 is None else u8.data_ptr(),
                                            self.xi.data_ptr(), self.xc.data_ptr(), self.yi.data_ptr(), self.yc.data_ptr(),
                                            t, self.src_h, self.src_w, self.crop, self.out_h, self.out_w, int(flip),
                                            0 if layout == "nchw" else 1, mean, std,
                                            torch.cuda.current_stream().cuda_stream), "phnet_preprocess_u8")
        else:
            rows, pitch = self.frame_shape
            check(lib().phnet_preprocess_yuv(frames_u8.data_ptr(), out.data_ptr(), None if u8 is None else u8.data_ptr(),
                                             self.xi.data_ptr(), self.xc.data_ptr(), self.yi.data_ptr(), self.yc.data_ptr(),
                                             t, self.src_h, self.src_w, self.crop, self.out_h, self.out_w, int(flip),
                                             0 if layout == "nchw" else 1, _FORMATS[self.pixel_format], rows * pitch, pitch,
                                             self.surface_rows * pitch, ctypes.cast(self._csc, ctypes.c_void_p), mean, std,
                                             torch.cuda.current_stream().cuda_stream), "phnet_preprocess_yuv")
        if augment is not None:
            if self._augmenter is None:
                from phnet_amd.libs.dataset.openlane.augment import ClipAugmenter
                self._augmenter = ClipAugmenter.for_preprocessor(self)
            return self._augmenter(u8, augment, layout=layout, out=out, return_u8=return_u8)
        return (out, u8) if return_u8 else out


def multibatch_collate_fn(batch):
    """datasetOL.py:11-17 for already pre-processed samples: [([{img, lane_line}, ...], info), ...] -> (frames [B,T,3,H,W],
    lanes [B,T,4,6+S], infos)."""
    outs, infos = [s[0] for s in batch], [s[1] for s in batch]
    frames = torch.stack([torch.stack([d["img"] for d in sample]) for sample in outs])
    lanes = torch.stack([torch.stack([torch.as_tensor(d["lane_line"]) for d in sample]) for sample in outs])
    return frames, lanes, infos
