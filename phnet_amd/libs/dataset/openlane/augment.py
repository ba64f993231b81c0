"""Training augmentation on the GPU: the resized 8-bit clip and its lane annotations go through the same per-frame random flip, colour
change, dropout and affine warp, the image in ONE launch (csrc/augment.hip, `phnet_augment_u8`) and the labels inside the target launch
(csrc/lane_targets.hip rule 0b, `phnet_lane_targets_aug`).  This stands where the reference's imgaug pipeline stands, between the resize
(`ClipPreprocessor`) and the label rows (`TargetEncoder`): libs/dataset/openlane/transforms.py:190-249, `mode_transform` 'basic' / 'complex',
run there per frame on CPU workers.  All parameters live in a device table (`AugmentParams`), so both launches can be captured in a graph
and a replay uses whatever `copy_into` put into the table since.  No CPU path.

Built: HorizontalFlip, ChannelShuffle, MultiplyAndAddToBrightness, AddToHueAndSaturation, EdgeDetect / DirectedEdgeDetect, Dropout,
CoarseDropout, MotionBlur / MedianBlur / GaussianBlur and Affine (constant fill 0), in the reference's order with the affine last, by the
numbered rules of include/phnet_hip.h.  The five neighbourhood ops (rule 7) live in a second table, `AugmentParams.stencil`; a frame that
has one takes a staging pass (csrc/augment_stencil.hip, a second launch inside `phnet_augment_stencil_u8`) and the warp reads its taps
from the staged image.  `AugmentSampler(..., neighbourhood=True)` draws them; the default does not, and keeps the earlier stream of draws.

Line clipping (clip_out_of_image_() on the line strings) is `TargetEncoder(..., clip=True)`, rule 0c of the target launch: an affine
moves more points out of the image, so the augmented pipeline should run with it.  The reference's loop that retries a failing draw up
to 30 times (transforms.py:63-75) is dead code for every input the rules accept - it retries only when transform_annotation raises, and
with finite points it cannot (DESIGN.md "Training augmentation") - so nothing stands in its place but `frag_count=` of the encoder: one
integer per frame, 0 where the draw left no lane.

PARITY UNPINNED: imgaug, cv2 and skimage are not installed here and the reference ships no image fixture; cv2.warpAffine's tables,
imgaug's colour-space round trips and cv2's fixed-point filters cannot be reproduced bit for bit.  The kernels are held exactly to a
numpy restatement of their own rules (tests/augment_cases.py, tests/stencil_cases.py); op order, fill, borders, ranges and the meaning
of each parameter follow imgaug's and OpenCV's documentation (the border defaults - reflect-101 for filter2D and GaussianBlur,
replicate for medianBlur - are written down from memory).  The sampler makes no claim that its stream of draws equals imgaug's."""
import ctypes
import math
from typing import Optional, Sequence

import numpy as np
import torch

from phnet_amd import hip_ops as K

COLS = K.AUGMENT_TABLE_COLS
STENCIL_COLS = K.AUGMENT_STENCIL_COLS
# columns of the i32 table (include/phnet_hip.h)
PERM0, MULQ, ADD, VALUE, MODE, PER_CHANNEL, THRESH, GRID_H, GRID_W, SEED_LO, SEED_HI = 0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12
DROP_MODES = {"none": 0, "pixel": 1, "coarse": 2}
# columns of the i32 stencil table (include/phnet_hip.h rule 7)
EDGE_ON, EDGE0, BLUR_KIND, BLUR_K, BLUR_W0 = 0, 1, 10, 11, 12
BLUR_KINDS = {"motion": 1, "median": 2, "gaussian": 3}
BLUR_SIZES = {"motion": (3, 5), "median": (3, 5), "gaussian": (3, 5, 7, 9)}
Q12, Q8 = 4096, 256


def affine_matrices(out_h: int, out_w: int, rotate_deg: float = 0.0, scale: float = 1.0, translate_x: float = 0.0, translate_y: float = 0.0):
    """(fwd, inv), float64 [6] each, row-major 2 x 3.  Convention: pixel centres at integer coordinates, x to the right, y DOWN;
    fwd maps a point of the un-warped (source) image to the warped (output) image,
        fwd = T(c) . T(translate_x * W, translate_y * H) . R(theta) . S(scale) . T(-c),    c = ((W - 1) / 2, (H - 1) / 2),
    with R(theta) = [[cos, -sin], [sin, cos]]: theta = rotate_deg is positive CLOCKWISE on the screen (imgaug's Affine); translations are
    fractions of the image size.  inv = fwd^-1 in closed form (R^T / scale), in double: the matrix the image kernel applies to output
    pixels.  The labels take fwd."""
    if not (scale > 0 and all(math.isfinite(v) for v in (rotate_deg, scale, translate_x, translate_y))):
        raise ValueError("affine_matrices: finite parameters and scale > 0 expected")
    cx, cy = (out_w - 1) / 2.0, (out_h - 1) / 2.0
    tx, ty = translate_x * out_w, translate_y * out_h
    th = math.radians(rotate_deg)
    c, s = math.cos(th), math.sin(th)
    a00, a01, a10, a11 = scale * c, -scale * s, scale * s, scale * c
    fwd = np.array([a00, a01, (cx + tx) - (a00 * cx + a01 * cy), a10, a11, (cy + ty) - (a10 * cx + a11 * cy)], np.float64)
    b00, b01, b10, b11 = c / scale, s / scale, -s / scale, c / scale
    inv = np.array([b00, b01, cx - (b00 * (cx + tx) + b01 * (cy + ty)), b10, b11, cy - (b10 * (cx + tx) + b11 * (cy + ty))], np.float64)
    return fwd, inv


def dropout_threshold(p: float) -> int:
    """The uint32 threshold of phnet_rng_keep for a drop probability p (as phnet_make_rng forms it): min(2^32 - 1, floor(p * 2^32))."""
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"dropout p = {p} outside [0, 1]")
    return int(min(4294967295.0, math.floor(p * 4294967296.0)))


def edge_kernel(alpha: float) -> np.ndarray:
    """imgaug's EdgeDetect: (1 - alpha) * identity + alpha * [[0, 1, 0], [1, -4, 1], [0, 1, 0]], float64 [3, 3].  Its weights sum to
    1 - alpha: the op darkens a flat image, as imgaug's does."""
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"edge_kernel: alpha = {alpha} outside [0, 1]")
    ident = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], np.float64)
    return (1.0 - alpha) * ident + alpha * np.array([[0, 1, 0], [1, -4, 1], [0, 1, 0]], np.float64)


def directed_edge_kernel(alpha: float, direction: float) -> np.ndarray:
    """imgaug's DirectedEdgeDetect: direction in [0, 1] is a turn (0 = up, clockwise); each of the eight neighbours is weighted by
    (1 - angle / 180 deg)^4 of the angle between it and the direction vector, the weights are normalised to sum 1 and negated, the
    centre is 1, and the result is blended with the identity by alpha.  float64 [3, 3], sum 1 - alpha."""
    if not 0.0 <= alpha <= 1.0 or not math.isfinite(direction):
        raise ValueError(f"directed_edge_kernel: alpha = {alpha} outside [0, 1] or direction {direction} not finite")
    rad = math.radians(int(direction * 360) % 360)
    dvec = np.array([math.cos(rad - 0.5 * math.pi), math.sin(rad - 0.5 * math.pi)])
    effect = np.zeros((3, 3), np.float64)
    for y in (-1, 0, 1):
        for x in (-1, 0, 1):
            if (x, y) != (0, 0):
                cell = np.array([x, y], np.float64)
                cos = float(np.clip(np.dot(cell / np.linalg.norm(cell), dvec), -1.0, 1.0))
                effect[y + 1, x + 1] = (1.0 - math.degrees(math.acos(cos)) / 180.0) ** 4
    effect = -effect / effect.sum()
    effect[1, 1] = 1.0
    ident = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], np.float64)
    return (1.0 - alpha) * ident + alpha * effect


def motion_kernel(k: int, angle: float, direction: float) -> np.ndarray:
    """imgaug's MotionBlur: a vertical line through the centre of a k x k matrix whose weights run linearly from d to 1 - d,
    d = (direction + 1) / 2 with direction in [-1, 1], rotated by `angle` degrees (clockwise, y down) about the centre with bilinear
    sampling and zero fill, normalised to sum 1.  float64 [k, k]."""
    if k not in BLUR_SIZES["motion"] or not math.isfinite(angle) or not -1.0 <= direction <= 1.0:
        raise ValueError(f"motion_kernel: k in {BLUR_SIZES['motion']}, a finite angle and direction in [-1, 1] expected")
    d = (direction + 1.0) / 2.0
    line = np.zeros((k, k), np.float64)
    line[:, k // 2] = np.linspace(d, 1.0 - d, k)
    th, c = math.radians(angle), (k - 1) / 2.0
    cs, sn = math.cos(th), math.sin(th)
    out = np.zeros((k, k), np.float64)
    for y in range(k):
        for x in range(k):
            sx, sy = cs * (x - c) + sn * (y - c) + c, -sn * (x - c) + cs * (y - c) + c         # the output -> source rotation
            x0, y0 = math.floor(sx), math.floor(sy)
            for yy, wy in ((y0, 1.0 - (sy - y0)), (y0 + 1, sy - y0)):
                for xx, wx in ((x0, 1.0 - (sx - x0)), (x0 + 1, sx - x0)):
                    if 0 <= xx < k and 0 <= yy < k:
                        out[y, x] += wy * wx * line[yy, xx]
    return out / out.sum()                                          # the centre keeps weight 1/2 under every rotation: sum > 0


def gaussian_kernel(sigma: float) -> Optional[np.ndarray]:
    """The k one-dimensional weights of imgaug's GaussianBlur (its cv2 backend): k = 3.3 sigma for sigma < 3, else 2.9 sigma,
    floored, at least 5, made odd, at most 9; exp(-x^2 / (2 sigma^2)) normalised to sum 1.  None for sigma < 0.001: no blur."""
    if not (math.isfinite(sigma) and sigma >= 0.0):
        raise ValueError(f"gaussian_kernel: sigma = {sigma} is not a finite non-negative number")
    if sigma < 0.001:
        return None
    k = max(int(math.floor((3.3 if sigma < 3.0 else 2.9) * sigma)), 5)
    k = min(k + 1 if k % 2 == 0 else k, 9)
    x = np.arange(k, dtype=np.float64) - k // 2
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return g / g.sum()


def quantise_kernel(weights, one: int) -> np.ndarray:
    """Float weights -> integers on the scale `one` (Q12: 4096, Q8: 256), each rounded to nearest; the largest-magnitude weight then
    absorbs the remainder, so that the integers sum to rint(sum(weights) * one) exactly - 4096 or 256 for a kernel that sums to 1: a
    flat image stays flat under it."""
    w = np.asarray(weights, np.float64)
    q = np.rint(w * one).astype(np.int64)
    q.reshape(-1)[int(np.argmax(np.abs(w)))] += int(np.rint(w.sum() * one)) - int(q.sum())
    return q


class AugmentParams:
    """The per-frame table of T frames: flip2 i32 [T], inv f64 [T,6] (image: output -> source), fwd f64 [T,6] (labels: source -> output),
    table i32 [T,16] and, optionally, stencil i32 [T,40], the neighbourhood ops (columns: include/phnet_hip.h); stencil = None means no
    frame has one.  Build it on the host with `identity` or `build` (which validate), move it with `to`, refresh a captured one with
    `copy_into`."""

    def __init__(self, flip2: torch.Tensor, inv: torch.Tensor, fwd: torch.Tensor, table: torch.Tensor, stencil: Optional[torch.Tensor] = None):
        t = flip2.shape[0] if flip2.dim() == 1 else -1
        if (flip2.dtype, inv.dtype, fwd.dtype, table.dtype) != (torch.int32, torch.float64, torch.float64, torch.int32) or \
                tuple(inv.shape) != (t, 6) or tuple(fwd.shape) != (t, 6) or tuple(table.shape) != (t, COLS):
            raise ValueError("AugmentParams: flip2 i32 [T], inv f64 [T,6], fwd f64 [T,6], table i32 [T,16] expected")
        if stencil is not None and (stencil.dtype != torch.int32 or tuple(stencil.shape) != (t, STENCIL_COLS) or stencil.device != flip2.device):
            raise ValueError(f"AugmentParams: stencil i32 [T,{STENCIL_COLS}] on the device of the other tensors expected")
        self.flip2, self.inv, self.fwd, self.table, self.stencil = flip2, inv, fwd, table, stencil

    def __len__(self):
        return self.flip2.shape[0]

    @property
    def device(self):
        return self.flip2.device

    def tensors(self):
        """(flip2, inv, fwd, table), and stencil behind them when present."""
        return (self.flip2, self.inv, self.fwd, self.table) + (() if self.stencil is None else (self.stencil,))

    @classmethod
    def identity(cls, T: int, pin: bool = False, stencil: Optional[bool] = None) -> "AugmentParams":
        """T neutral frames: no flip, identity matrices, perm 0 1 2, mq 256, add 0, value 0, no dropout; stencil=True: with an all-zero
        stencil table (the table a captured graph reads, to be refreshed by `copy_into`)."""
        return cls.build([{}] * int(T), 1, 1, pin=pin, stencil=stencil)

    @staticmethod
    def _stencil_row(f: int, d: dict) -> Optional[np.ndarray]:
        """The stencil row of one frame's dict, or None when it has neither `edge` nor `blur`."""
        edge, blur = d.get("edge"), d.get("blur")
        if edge is None and blur is None:
            return None
        row = np.zeros((STENCIL_COLS,), np.int64)
        if edge is not None:
            if not isinstance(edge, dict) or set(edge) != {"weights"}:
                raise ValueError(f"frame {f}: edge = dict(weights = 3 x 3 floats) expected, got {edge}")
            w = np.asarray(edge["weights"], np.float64)
            if w.shape != (3, 3) or not np.isfinite(w).all() or np.abs(w).max() > 16.0:
                raise ValueError(f"frame {f}: edge weights must be 3 x 3 finite floats within [-16, 16]")
            row[EDGE_ON], row[EDGE0:EDGE0 + 9] = 1, quantise_kernel(w, Q12).reshape(-1)
        if blur is not None:
            if not isinstance(blur, dict) or set(blur) - {"kind", "k", "weights"} or blur.get("kind") not in BLUR_KINDS:
                raise ValueError(f"frame {f}: blur = dict(kind 'motion' | 'median' | 'gaussian', k, weights) expected, got {blur}")
            kind, k = blur["kind"], blur.get("k")
            if not isinstance(k, (int, np.integer)) or int(k) not in BLUR_SIZES[kind]:
                raise ValueError(f"frame {f}: {kind} blur needs k in {BLUR_SIZES[kind]}, got {k}")
            k = int(k)
            row[BLUR_KIND], row[BLUR_K] = BLUR_KINDS[kind], k
            if kind == "median":
                if blur.get("weights") is not None:
                    raise ValueError(f"frame {f}: a median blur takes no weights")
            else:
                w = np.asarray(blur.get("weights", ()), np.float64)
                shape = (k, k) if kind == "motion" else (k,)
                if w.shape != shape or not np.isfinite(w).all() or w.min() < 0.0 or abs(w.sum() - 1.0) > 1e-6:
                    raise ValueError(f"frame {f}: {kind} blur with k = {k} needs {' x '.join(map(str, shape))} non-negative weights that sum to 1")
                row[BLUR_W0:BLUR_W0 + w.size] = quantise_kernel(w, Q12 if kind == "motion" else Q8).reshape(-1)
        return row

    @classmethod
    def build(cls, frames: Sequence[dict], out_h: int, out_w: int, pin: bool = False, stencil: Optional[bool] = None) -> "AugmentParams":
        """One dict per frame; every key is optional and neutral when absent:
            flip (bool), perm (a permutation of 0, 1, 2), mul (float in [0, 256]), add (int in [-255, 255]), value (int in [-255, 255]:
            hue and saturation), edge = dict(weights 3 x 3 floats: `edge_kernel`, `directed_edge_kernel`), dropout = dict(mode "pixel" |
            "coarse", p in [0, 1], per_channel bool, seed uint64, grid (gh, gw) for "coarse", each in [1, 32768]), blur = dict(kind
            "motion" | "median" | "gaussian", k odd (3, 5; gaussian also 7, 9), weights k x k (`motion_kernel`) / k (`gaussian_kernel`) /
            none), rotate (degrees, clockwise), scale (> 0), translate (tx, ty as fractions of W, H).
        stencil: None - the stencil table is present iff a frame has `edge` or `blur`; True - always present (all-zero rows for the
        other frames); False - never, and such a frame is an error.
        Raises ValueError on anything else: the kernels cannot report a bad table, they only clamp."""
        n = len(frames)
        flip2, table = np.zeros((n,), np.int32), np.zeros((n, COLS), np.int32)
        inv, fwd = np.zeros((n, 6), np.float64), np.zeros((n, 6), np.float64)
        sten, any_stencil = np.zeros((n, STENCIL_COLS), np.int32), False
        known = {"flip", "perm", "mul", "add", "value", "dropout", "rotate", "scale", "translate", "edge", "blur"}
        for f, d in enumerate(frames):
            if set(d) - known:
                raise ValueError(f"frame {f}: unknown keys {sorted(set(d) - known)}")
            srow = cls._stencil_row(f, d)
            if srow is not None:
                if stencil is False:
                    raise ValueError(f"frame {f}: edge / blur given with stencil=False")
                sten[f], any_stencil = srow, True
            flip2[f] = 1 if d.get("flip", False) else 0
            perm = [int(v) for v in d.get("perm", (0, 1, 2))]
            if sorted(perm) != [0, 1, 2]:
                raise ValueError(f"frame {f}: perm {perm} is not a permutation of 0, 1, 2")
            mul, add, value = float(d.get("mul", 1.0)), d.get("add", 0), d.get("value", 0)
            if not (0.0 <= mul <= 256.0) or int(add) != add or int(value) != value or not (-255 <= add <= 255 and -255 <= value <= 255):
                raise ValueError(f"frame {f}: mul {mul} outside [0, 256], or add {add} / value {value} not an integer in [-255, 255]")
            table[f, PERM0:PERM0 + 3] = perm
            table[f, MULQ], table[f, ADD], table[f, VALUE] = int(np.rint(mul * 256.0)), int(add), int(value)
            table[f, GRID_H] = table[f, GRID_W] = 1
            drop = d.get("dropout")
            if drop is not None:
                if set(drop) - {"mode", "p", "per_channel", "seed", "grid"} or drop.get("mode") not in ("pixel", "coarse"):
                    raise ValueError(f"frame {f}: dropout = dict(mode 'pixel' | 'coarse', p, per_channel, seed, grid) expected, got {drop}")
                gh, gw = (int(v) for v in drop.get("grid", (1, 1)))
                if not (1 <= gh <= K.AUGMENT_MAX_SIDE and 1 <= gw <= K.AUGMENT_MAX_SIDE) or (drop["mode"] == "coarse" and "grid" not in drop):
                    raise ValueError(f"frame {f}: coarse dropout needs grid = (gh, gw), each in [1, {K.AUGMENT_MAX_SIDE}]")
                seed = int(drop.get("seed", 0))
                if not 0 <= seed < 1 << 64:
                    raise ValueError(f"frame {f}: seed must be a uint64")
                words = np.array([dropout_threshold(float(drop.get("p", 0.0))), seed & 0xffffffff, seed >> 32], np.uint32).view(np.int32)
                table[f, MODE], table[f, PER_CHANNEL] = DROP_MODES[drop["mode"]], 1 if drop.get("per_channel", False) else 0
                table[f, THRESH], table[f, SEED_LO], table[f, SEED_HI] = words
                table[f, GRID_H], table[f, GRID_W] = gh, gw
            tx, ty = d.get("translate", (0.0, 0.0))
            if any(k in d for k in ("rotate", "scale", "translate")):
                fwd[f], inv[f] = affine_matrices(out_h, out_w, float(d.get("rotate", 0.0)), float(d.get("scale", 1.0)), float(tx), float(ty))
            else:
                fwd[f] = inv[f] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
        arrays = (flip2, inv, fwd, table) + ((sten,) if stencil or (stencil is None and any_stencil) else ())
        tensors = [torch.from_numpy(a) for a in arrays]
        return cls(*[x.pin_memory() for x in tensors] if pin else tensors)

    def to(self, device, non_blocking: bool = False) -> "AugmentParams":
        return AugmentParams(*[x.to(device, non_blocking=non_blocking) for x in self.tensors()])

    def copy_into(self, device_params: "AugmentParams", non_blocking: bool = True) -> "AugmentParams":
        """Overwrite the tensors of `device_params` (the table a captured graph reads) with these, in place; returns it.  A table
        without a stencil clears the stencil of `device_params`; one with a stencil needs `device_params` to have one."""
        if len(device_params) != len(self):
            raise ValueError(f"copy_into: a table of {len(device_params)} frames cannot take {len(self)}")
        if self.stencil is not None and device_params.stencil is None:
            raise ValueError("copy_into: the destination has no stencil table (build it with stencil=True)")
        for dst, src in zip(device_params.tensors(), self.tensors()):
            dst.copy_(src, non_blocking=non_blocking)
        if self.stencil is None and device_params.stencil is not None:
            device_params.stencil.zero_()
        return device_params

    def numpy(self):
        """dict(flip2, inv, fwd, table[, stencil]) of numpy arrays (a device table is copied to the host)."""
        return {k: v.detach().cpu().numpy() for k, v in zip(("flip2", "inv", "fwd", "table", "stencil"), self.tensors())}


# the reference's transforms.py:190-249, for the ops this module has: (probability, parameter ranges)
RECIPES = {
    "basic": dict(flip=0.5, shuffle=0.0, brightness=0.0, hue_sat=0.0, dropout=0.0, affine=0.7, rotate=10.0, scale=(0.8, 1.2), translate=0.1),
    "complex": dict(flip=0.1, shuffle=0.1, brightness=0.1, hue_sat=0.1, dropout=0.1, affine=0.1, rotate=5.0, scale=(0.9, 1.1), translate=0.1),
}
BRIGHTNESS_MUL, BRIGHTNESS_ADD, HUE_SAT_VALUE = (0.9, 1.1), (-10, 10), (-10, 10)
DROPOUT_P, COARSE_SIZE_PERCENT, COARSE_MIN_SIZE = (0.0, 0.05), (0.02, 0.25), 3
DROPOUT_PER_CHANNEL, COARSE_PER_CHANNEL = 0.5, 0.2
# the two OneOf groups of neighbourhood ops of 'complex' (transforms.py:220-238)
NEIGHBOURHOOD_P = dict(edge=0.1, blur=0.1)
EDGE_ALPHA, EDGE_DIRECTION = (0.0, 0.2), (0.0, 1.0)
BLUR_K_RANGE, MOTION_ANGLE, MOTION_DIRECTION, GAUSSIAN_SIGMA = (3, 5), (0.0, 360.0), (-1.0, 1.0), (0.0, 3.0)


class AugmentSampler:
    """Draws the parameters of `mode` = "basic" | "complex" (transforms.py:190-249) with a seeded numpy Generator.  per = "frame" (the
    reference: imgaug runs per frame, every frame draws afresh) or "clip" (one draw shared by the frames of a clip: temporally coherent).
    neighbourhood = True adds, to "complex", its two OneOf groups of neighbourhood ops (EdgeDetect / DirectedEdgeDetect behind the hue,
    MotionBlur / MedianBlur / GaussianBlur behind the dropout, p = 0.1 each), and every table it samples carries a stencil; with the
    default False those draws are not made and the stream of draws is the one this class has always produced for a seed."""

    def __init__(self, mode: str, out_h: int, out_w: int, seed: int, per: str = "frame", neighbourhood: bool = False):
        if mode not in RECIPES or per not in ("frame", "clip"):
            raise ValueError(f"mode must be one of {sorted(RECIPES)} and per 'frame' or 'clip', got {mode!r}, {per!r}")
        self.mode, self.per, self.out_h, self.out_w = mode, per, int(out_h), int(out_w)
        self.neighbourhood = bool(neighbourhood)
        self.rng = np.random.default_rng(seed)

    def draw(self) -> dict:
        """One frame's parameters, as a dict for AugmentParams.build, plus "ops": the names of the ops this draw switched on."""
        r, g, d, ops = RECIPES[self.mode], self.rng, {}, []
        on = lambda name: g.random() < r[name]                                          # noqa: E731
        if on("flip"):
            d["flip"] = True; ops.append("flip")
        if on("shuffle"):
            d["perm"] = tuple(int(v) for v in g.permutation(3)); ops.append("shuffle")
        if on("brightness"):
            d["mul"], d["add"] = float(g.uniform(*BRIGHTNESS_MUL)), int(g.integers(BRIGHTNESS_ADD[0], BRIGHTNESS_ADD[1] + 1)); ops.append("brightness")
        if on("hue_sat"):
            d["value"] = int(g.integers(HUE_SAT_VALUE[0], HUE_SAT_VALUE[1] + 1)); ops.append("hue_sat")
        groups = self.neighbourhood and self.mode == "complex"
        if groups and g.random() < NEIGHBOURHOOD_P["edge"]:
            alpha = float(g.uniform(*EDGE_ALPHA))
            if g.random() < 0.5:                                                        # OneOf
                d["edge"] = dict(weights=edge_kernel(alpha)); ops.append("edge")
            else:
                d["edge"] = dict(weights=directed_edge_kernel(alpha, float(g.uniform(*EDGE_DIRECTION)))); ops.append("directed_edge")
        if on("dropout"):
            seed = int(g.integers(0, 1 << 64, dtype=np.uint64))
            if g.random() < 0.5:                                                        # OneOf
                d["dropout"] = dict(mode="pixel", p=float(g.uniform(*DROPOUT_P)), per_channel=bool(g.random() < DROPOUT_PER_CHANNEL), seed=seed)
            else:
                pct = float(g.uniform(*COARSE_SIZE_PERCENT))
                grid = tuple(min(n, max(int(n * pct), COARSE_MIN_SIZE)) for n in (self.out_h, self.out_w))
                d["dropout"] = dict(mode="coarse", p=float(g.uniform(*DROPOUT_P)), per_channel=bool(g.random() < COARSE_PER_CHANNEL), seed=seed,
                                    grid=grid)
            ops.append("dropout")
        if groups and g.random() < NEIGHBOURHOOD_P["blur"]:
            which = int(g.integers(0, 3))                                               # OneOf
            if which == 0:
                k = int(g.integers(BLUR_K_RANGE[0], BLUR_K_RANGE[1] + 1)) | 1                       # an even k is raised by one
                d["blur"] = dict(kind="motion", k=k, weights=motion_kernel(k, float(g.uniform(*MOTION_ANGLE)), float(g.uniform(*MOTION_DIRECTION))))
                ops.append("motion_blur")
            elif which == 1:
                d["blur"] = dict(kind="median", k=int(g.integers(BLUR_K_RANGE[0], BLUR_K_RANGE[1] + 1)) | 1); ops.append("median_blur")
            else:
                weights = gaussian_kernel(float(g.uniform(*GAUSSIAN_SIGMA)))
                if weights is not None:                                                 # sigma < 0.001: no blur
                    d["blur"] = dict(kind="gaussian", k=len(weights), weights=weights)
                ops.append("gaussian_blur")
        if on("affine"):
            d["translate"] = (float(g.uniform(-r["translate"], r["translate"])), float(g.uniform(-r["translate"], r["translate"])))
            d["rotate"], d["scale"] = float(g.uniform(-r["rotate"], r["rotate"])), float(g.uniform(*r["scale"]))
            ops.append("affine")
        d["ops"] = tuple(ops)
        return d

    def sample(self, T: int) -> AugmentParams:
        """The table of one clip of T frames, on the host (pinned where a device is present: copy with non_blocking=True)."""
        draws = [self.draw() for _ in range(int(T))] if self.per == "frame" else [self.draw()] * int(T)
        frames = [{k: v for k, v in d.items() if k != "ops"} for d in draws]
        return AugmentParams.build(frames, self.out_h, self.out_w, pin=torch.cuda.is_available(), stencil=self.neighbourhood)


class ClipAugmenter:
    """The image launch: resized uint8 frames [T,out_h,out_w,3] + an AugmentParams on the same device -> the normalised clip.  With a
    stencil table in the params: the staging launch of the neighbourhood ops and the image launch (phnet_augment_stencil_u8), with one
    staging buffer per (T, device) that this object keeps."""

    def __init__(self, out_h: int, out_w: int, mean: Sequence[float] = (0.485, 0.456, 0.406), std: Sequence[float] = (0.229, 0.224, 0.225),
                 device="cuda"):
        self.out_h, self.out_w, self.device = int(out_h), int(out_w), torch.device(device)
        if not (1 <= self.out_h <= K.AUGMENT_MAX_SIDE and 1 <= self.out_w <= K.AUGMENT_MAX_SIDE):
            raise ValueError(f"ClipAugmenter: {out_h} x {out_w} outside 1 .. {K.AUGMENT_MAX_SIDE}")
        if len(mean) != 3 or len(std) != 3 or any(float(v) == 0.0 for v in std):
            raise ValueError("ClipAugmenter: three means and three non-zero stds expected")
        self._mean = (ctypes.c_float * 3)(*[float(v) for v in mean])
        self._std = (ctypes.c_float * 3)(*[float(v) for v in std])
        self._staged = {}                                           # stencil: the staged 8-bit frames per (T, device)

    @classmethod
    def for_preprocessor(cls, pre) -> "ClipAugmenter":
        """The augmenter behind a ClipPreprocessor: same output size, mean / std and device."""
        return cls(pre.out_h, pre.out_w, mean=tuple(pre._mean), std=tuple(pre._std), device=pre.xi.device)

    def __call__(self, frames_u8: torch.Tensor, params: AugmentParams, layout: str = "nchw", out: Optional[torch.Tensor] = None,
                 return_u8: bool = False, out_u8: Optional[torch.Tensor] = None):
        """-> float32 [T,3,out_h,out_w] ("nchw") or [T,out_h,out_w,4] ("nhwc4"); with return_u8 also the augmented 8-bit frames.  out /
        out_u8: buffers to write into - then (with a stencil table, after one call of the same T) nothing is allocated and the call can be
        captured in a graph."""
        if frames_u8.dim() != 4 or tuple(frames_u8.shape[1:]) != (self.out_h, self.out_w, 3):
            raise ValueError(f"ClipAugmenter: frames [T,{self.out_h},{self.out_w},3] expected, got {tuple(frames_u8.shape)}")
        if not isinstance(params, AugmentParams) or len(params) != frames_u8.shape[0]:
            raise ValueError(f"ClipAugmenter: an AugmentParams of {frames_u8.shape[0]} frames expected")
        if not frames_u8.is_cuda or params.device != frames_u8.device:
            raise RuntimeError("ClipAugmenter: frames and params on the same CUDA(HIP) device expected; phnet_amd has no CPU path")
        if return_u8 and out_u8 is None:
            out_u8 = torch.empty_like(frames_u8)
        staged = None
        if params.stencil is not None:
            key = (frames_u8.shape[0], frames_u8.device)
            staged = self._staged.get(key)
            if staged is None:
                staged = self._staged[key] = torch.empty_like(frames_u8, memory_format=torch.contiguous_format)
        res = K.augment_u8(frames_u8, params.flip2, params.inv, params.table, self._mean, self._std, layout=layout, out=out, out_u8=out_u8,
                           stencil=params.stencil, staged=staged)
        return (res, out_u8) if return_u8 else res
