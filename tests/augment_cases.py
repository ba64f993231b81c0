"""Training augmentation (csrc/augment.hip, csrc/lane_targets.hip rule 0b): a restatement of the numbered rules of include/phnet_hip.h in
numpy - int64 where the kernel computes in int32, float64 where it computes in float64, nothing contracted - and the cases.

Image half: `augment(frames, flip2, inv, table)` gives the augmented 8-bit image, integer for integer, and an `info` dict that records
which branches the pixels took, so tests/test_augment_cpu.py can show without a GPU that the cases reach what they are for;
`epilogue` is the shared q / 255, (v - mean) / std in float32.  Label half: `encode_frame_aug` puts rule 0b in front of the restatement
of tests/target_cases.py, which it imports and does not copy.  PARITY UNPINNED against imgaug / cv2 (phnet_amd/libs/dataset/openlane/
augment.py): this file restates the project's own rules.

Shapes: the `tiny` geometry of target_cases (64 x 160, S = 36, R = 4) with T = 3, and one 37 x 53 image: 1961 pixels, not a multiple of
the 256-thread workgroup.  Its centre (26, 18) is integral, the tiny geometry's (79.5, 31.5) is not: both centre parities.
Every annotation coordinate is a multiple of 1/64."""
import functools
from unittest import mock

import numpy as np

from phnet_amd.libs.dataset.openlane.augment import AugmentParams
from tests import target_cases as C

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HUE = 24576
SHAPES = {"tiny": (3, 64, 160), "odd": (1, 37, 53)}               # name -> (T, H, W)


# ----------------------------------------------------------------------------------------------------- the restatement: image
def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def rng_keep(seed, idx, thresh):
    """phnet_rng_keep of csrc/common.h on a uint64 array of indices."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (idx.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        return (_mix64(z) >> np.uint64(32)) >= np.uint64(thresh)


def _row(table_row):
    """The clamps of the kernel on one table row -> dict."""
    r = [int(v) for v in table_row]
    u32 = lambda v: v & 0xffffffff                                                   # noqa: E731
    return dict(perm=[min(max(v, 0), 2) for v in r[0:3]], mq=min(max(r[3], 0), 65536), add=min(max(r[4], -255), 255),
                value=min(max(r[5], -255), 255), mode=r[6], per_channel=r[7] != 0, thresh=u32(r[8]), gh=min(max(r[9], 1), 32768),
                gw=min(max(r[10], 1), 32768), seed=(u32(r[12]) << 32) | u32(r[11]))


def colour(c, p, info):
    """Rule 4 on taps c int64 [N, 3]."""
    if p["perm"] != [0, 1, 2]:
        c = c[:, p["perm"]]
        info["perm"] += len(c)
    if p["mq"] != 256 or p["add"] != 0:
        V = c.max(axis=1)
        V2 = np.clip(((V * p["mq"] + 128) >> 8) + p["add"], 0, 255)
        black = V == 0
        Vs = np.where(black, 1, V)
        c = np.where(black[:, None], V2[:, None], (2 * c * V2[:, None] + Vs[:, None]) // (2 * Vs[:, None]))
        info["bright_black"] += int(black.sum()); info["bright_scaled"] += int((~black).sum())
        info["bright_clamped"] += int(((((V * p["mq"] + 128) >> 8) + p["add"] < 0) | ((((V * p["mq"] + 128) >> 8) + p["add"]) > 255)).sum())
    if p["value"] != 0:
        R, G, B = c[:, 0], c[:, 1], c[:, 2]
        V, mn = c.max(axis=1), c.min(axis=1)
        Cc = V - mn
        S = np.where(V == 0, 0, (510 * Cc + V) // (2 * np.where(V == 0, 1, V)))
        is_r, is_g = V == R, (V != R) & (V == G)
        base = np.where(is_r, 0, np.where(is_g, 8192, 16384))
        d = np.where(is_r, G - B, np.where(is_g, B - R, R - G))
        Cs = np.where(Cc == 0, 1, Cc)
        h = np.where(Cc == 0, 0, (base + ((d + Cs) * 8192 + Cs) // (2 * Cs) - 4096 + HUE) % HUE)
        S2 = np.clip(S + p["value"], 0, 255)
        C2 = (2 * V * S2 + 255) // 510
        dh = (p["value"] * (2 * HUE) + 255) // 510                                     # Python: floor
        h2 = (h + dh) % HUE                                                           # numpy: non-negative
        i, f = h2 >> 12, h2 & 4095
        lo, q, t = V - C2, V - ((C2 * f + 2048) >> 12), V - ((C2 * (4096 - f) + 2048) >> 12)
        pick = lambda a: np.choose(i, a)                                              # noqa: E731
        c = np.stack([pick([V, q, lo, lo, t, V]), pick([t, V, V, q, lo, lo]), pick([lo, lo, t, V, V, q])], axis=1)
        info["hsv_grey"] += int((Cc == 0).sum()); info["hsv_black"] += int((V == 0).sum())
        info["hsv_max"] |= {n for n, m in (("r", is_r), ("g", is_g), ("b", ~is_r & ~is_g)) if (m & (Cc != 0)).any()}
        info["hsv_sextants"] |= set(np.unique(i[Cc != 0]).tolist())
        info["hsv_sat_clamped"] += int(((S + p["value"] < 0) | (S + p["value"] > 255)).sum())
        info["hsv_wrapped"] += int(((h + dh < 0) | (h + dh >= HUE)).sum())
    return c


def dropout(c, p, t, xt, yt, H, W, info):
    """Rule 5 on taps c [N, 3] at (xt, yt) of frame t."""
    if p["mode"] not in (1, 2):
        return c
    if p["mode"] == 1:
        e = (t * H + yt) * W + xt
    else:
        e = (t * p["gh"] + (yt * p["gh"]) // H) * p["gw"] + (xt * p["gw"]) // W
    if p["per_channel"]:
        keep = np.stack([rng_keep(p["seed"], e * 3 + k, p["thresh"]) for k in range(3)], axis=1)
    else:
        keep = np.repeat(rng_keep(p["seed"], e, p["thresh"])[:, None], 3, axis=1)
    info["dropped"] += int((~keep).sum()); info["drop_elems"] += keep.size
    return np.where(keep, c, 0)


def new_info():
    return dict(guard_fill=0, taps_outside=0, pixels_all_outside=0, one_tap=0, many_taps=0, perm=0, bright_black=0, bright_scaled=0,
                bright_clamped=0, hsv_grey=0, hsv_black=0, hsv_max=set(), hsv_sextants=set(), hsv_sat_clamped=0, hsv_wrapped=0, dropped=0,
                drop_elems=0, flipped_frames=0)


def augment(frames, flip2, inv, table):
    """frames u8 [T, H, W, 3] -> (augmented u8 [T, H, W, 3], info) by rules 1 - 6."""
    T, H, W, _ = frames.shape
    out = np.zeros_like(frames)
    info = new_info()
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for t in range(T):
        p, a = _row(table[t]), [float(v) for v in inv[t]]
        info["flipped_frames"] += int(flip2[t] != 0)
        u = ((a[0] * xs + a[1] * ys) + a[2]).ravel()                                   # rule 1
        v = ((a[3] * xs + a[4] * ys) + a[5]).ravel()
        with np.errstate(invalid="ignore"):
            ok = (u > -2.0) & (u < W + 1.0) & (v > -2.0) & (v < H + 1.0)               # rule 2 (False for NaN)
        info["guard_fill"] += int((~ok).sum())
        U = np.floor(np.where(ok, u, 0.0) * 32.0 + 0.5).astype(np.int64)
        Vq = np.floor(np.where(ok, v, 0.0) * 32.0 + 0.5).astype(np.int64)
        x0, fx, y0, fy = U >> 5, U & 31, Vq >> 5, Vq & 31
        acc = np.zeros((H * W, 3), np.int64)
        used = np.zeros(H * W, np.int64)
        for j in (0, 1):
            for k in (0, 1):
                xt, yt = x0 + k, y0 + j
                w = (fx if k else 32 - fx) * (fy if j else 32 - fy)
                inside = (xt >= 0) & (xt < W) & (yt >= 0) & (yt < H)
                live = ok & (w > 0)
                info["taps_outside"] += int((live & ~inside).sum())
                sel = np.nonzero(live & inside)[0]                                     # rule 3
                sx = np.where(flip2[t] != 0, W - 1 - xt[sel], xt[sel])
                c = frames[t, yt[sel], sx].astype(np.int64)
                c = colour(c, p, info)                                                 # rule 4
                c = dropout(c, p, t, xt[sel], yt[sel], H, W, info)                     # rule 5
                acc[sel] += w[sel, None] * c
                used[sel] += 1
        info["pixels_all_outside"] += int((ok & (used == 0)).sum())
        info["one_tap"] += int((used == 1).sum()); info["many_taps"] += int((used > 1).sum())
        q = (acc + 512) >> 10                                                          # rule 6
        assert q.min() >= 0 and q.max() <= 255
        out[t] = q.reshape(H, W, 3).astype(np.uint8)
    return out, info


def epilogue(u8, layout="nchw", mean=MEAN, std=STD):
    """The shared epilogue in float32: q / 255, then (v - mean) / std; NCHW [T,3,H,W] or NHWC4 [T,H,W,4] (fourth channel 0)."""
    v = u8.astype(np.float32) / np.float32(255.0)
    v = (v - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    assert v.dtype == np.float32
    if layout == "nchw":
        return np.ascontiguousarray(v.transpose(0, 3, 1, 2))
    return np.concatenate([v, np.zeros(v.shape[:3] + (1,), np.float32)], axis=3)


# ----------------------------------------------------------------------------------------------------- the restatement: labels
class _NumpyWithoutTheCast:
    """numpy as target_cases.encode_lane sees it while rule 0b's doubles pass through: encode_lane rounds every incoming coordinate to
    float32 first (its inputs are the kernel's float32 points), which must not happen to points that rules 0 and 0b already mapped."""
    float32 = staticmethod(lambda v: v)

    def __getattr__(self, name):
        return getattr(np, name)


def map_points(points, mapping, flip2, fwd, img_w):
    """Rule 0 (mapping of target_cases, or None), then rule 0b, on [(x, y)] float32 values -> [(x, y)] doubles."""
    out = []
    for x, y in points:
        x, y = float(np.float32(x)), float(np.float32(y))
        if mapping is not None:
            y = y - mapping["crop"]
            if mapping["flip"]:
                x = (mapping["src_w"] - 1.0) - x
            x, y = x * mapping["scale_x"], y * mapping["scale_y"]
        if flip2:
            x = (float(img_w) - 1.0) - x
        if fwd is not None:
            f = [float(v) for v in fwd]
            x, y = (f[0] * x + f[1] * y) + f[2], (f[3] * x + f[4] * y) + f[5]
        out.append((x, y))
    return out


def encode_frame_aug(lanes, img_h, img_w, S, R, flip2, fwd, mapping=None):
    """target_cases.encode_frame with rule 0b behind rule 0: (label float32 [R, 6+S], infos)."""
    plain = C.encode_lane

    def lane(points, h, w, ys, _mapping=None):
        mapped = map_points(points, mapping, flip2, fwd, img_w)
        with mock.patch.object(C, "np", _NumpyWithoutTheCast()):
            return plain(mapped, h, w, ys, None)

    with mock.patch.object(C, "encode_lane", lane):
        return C.encode_frame(lanes, img_h, img_w, S, R, mapping=None)


# ---------------------------------------------------------------------------------------------------------------- the cases
def _hand_pixels():
    """Colours that reach every colour branch: black (V = 0), greys (C = 0), white, the six saturated corners and one colour inside each
    hue sextant, and near-black / near-white values for the clamps."""
    return np.array([(0, 0, 0), (128, 128, 128), (7, 7, 7), (255, 255, 255), (255, 0, 0), (255, 255, 0), (0, 255, 0), (0, 255, 255),
                     (0, 0, 255), (255, 0, 255), (200, 90, 30), (120, 210, 40), (20, 220, 130), (30, 100, 240), (150, 40, 230),
                     (240, 20, 110), (250, 251, 252), (3, 2, 1), (255, 254, 0), (1, 0, 0), (90, 200, 200), (254, 10, 254)], np.uint8)


@functools.lru_cache(maxsize=None)
def frames(shape):
    """Seeded random bytes; the last frame is the hand image: the hand colours tiled over it."""
    T, H, W = SHAPES[shape]
    rng = np.random.default_rng({"tiny": 11, "odd": 12}[shape])
    f = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    hand = _hand_pixels()
    idx = (np.arange(H)[:, None] * 5 + np.arange(W)[None, :]) % len(hand)
    if T > 1:
        f[-1] = hand[idx]
    else:
        f[0, ::2] = hand[idx][::2]                                                    # every other row of the single image
    f.setflags(write=False)
    return f


def _drop(mode, p, per_channel, seed, grid=None):
    d = dict(mode=mode, p=p, per_channel=per_channel, seed=seed)
    if grid is not None:
        d["grid"] = grid
    return d


# name -> one dict for every frame, or a list of T dicts.  "Both ends of its range": the ranges of transforms.py:190-249
PARAM_SETS = {
    "identity": {},
    "perm_201": dict(perm=(2, 0, 1)), "perm_021": dict(perm=(0, 2, 1)),
    "bright_lo": dict(mul=0.9, add=-10), "bright_hi": dict(mul=1.1, add=10),
    "huesat_lo": dict(value=-10), "huesat_hi": dict(value=10),
    "flip2": dict(flip=True),
    "rot90": dict(rotate=90.0), "rot180": dict(rotate=180.0),
    "affine_pos": dict(rotate=7.3, scale=0.8, translate=(0.1, -0.1)), "affine_neg": dict(rotate=-7.3, scale=0.8, translate=(0.1, -0.1)),
    "affine_basic_lo": dict(rotate=-10.0, scale=0.8, translate=(-0.1, -0.1)), "affine_basic_hi": dict(rotate=10.0, scale=1.2, translate=(0.1, 0.1)),
    "translate_full": dict(translate=(1.0, 0.0)),
    "drop_p0": dict(dropout=_drop("pixel", 0.0, False, 5)),
    "drop_pixel": dict(dropout=_drop("pixel", 0.05, False, 0x0123456789abcdef)),
    "drop_pixel_per_channel": dict(dropout=_drop("pixel", 0.05, True, 0xfedcba9876543210)),
    "drop_coarse": dict(dropout=_drop("coarse", 0.3, False, 77, grid=(3, 5))),
    "everything": [dict(flip=True, perm=(1, 2, 0), mul=1.07, add=-6, value=9, dropout=_drop("coarse", 0.3, True, 1234567, grid=(3, 5)),
                        rotate=4.1, scale=1.08, translate=(-0.04, 0.07)),
                   dict(flip=False, perm=(2, 1, 0), mul=0.93, add=8, value=-7, dropout=_drop("pixel", 0.04, True, 99), rotate=-3.3, scale=0.92,
                        translate=(0.06, -0.03)),
                   dict(flip=True, perm=(0, 1, 2), mul=1.1, add=10, value=-10, dropout=_drop("pixel", 0.05, False, 2 ** 63 + 5), rotate=5.0,
                        scale=0.9, translate=(0.1, 0.1))],
}
# the label half runs the sets that move points.  rot90 is left to the image: it turns every lane into a nearly horizontal line, many
# points per y, which the function-of-y representation of the rows cannot hold
LABEL_SETS = ("identity", "flip2", "rot180", "affine_pos", "affine_neg", "affine_basic_lo", "affine_basic_hi", "translate_full", "everything")


@functools.lru_cache(maxsize=None)
def params(shape, name):
    """The AugmentParams (host) of a parameter set for a shape."""
    T, H, W = SHAPES[shape]
    spec = PARAM_SETS[name]
    return AugmentParams.build(spec[:T] if isinstance(spec, list) else [spec] * T, H, W)


@functools.lru_cache(maxsize=None)
def expected(shape, name):
    """(augmented u8, info) of a parameter set on the frames of a shape, by the restatement; read-only."""
    p = params(shape, name).numpy()
    out, info = augment(frames(shape), p["flip2"], p["inv"], p["table"])
    out.setflags(write=False)
    return out, info


# ---- labels: the tiny geometry, T = 3 frames of lanes, the identity map of rule 0 (annotations in output pixels)
LABEL_MARGIN = 1e-3                           # every warped sample is at least this far from 0 and img_w, under every label set
LABEL_MIN_DY = 0.25                           # adjacent warped points of a lane are at least this far apart in y


def _lane(rng, H, W):
    n = int(rng.integers(3, 12))
    return C.curve(W * rng.uniform(0.15, 0.85), W * rng.uniform(-0.3, 0.3), W * rng.uniform(-0.1, 0.1), H * rng.uniform(0.75, 1.0),
                   H * rng.uniform(0.05, 0.3), n)


def label_margins(lane, H, W, S):
    """(least |x| / |x - W| distance of a sample, least y gap of adjacent warped points) of a lane over every label set and frame."""
    ys, far, gap = C.offsets(H, S), np.inf, np.inf
    for name in LABEL_SETS:
        p = params("tiny", name).numpy()
        for t in range(SHAPES["tiny"][0]):
            pts = map_points(lane, None, p["flip2"][t], p["fwd"][t], W)
            sy = sorted(y for _, y in pts)
            gap = min(gap, min(b - a for a, b in zip(sy[:-1], sy[1:])))
            with mock.patch.object(C, "np", _NumpyWithoutTheCast()):
                _, info = C.encode_lane(pts, H, W, ys, None)
            far = min([far] + [min(abs(x), abs(x - W)) for x in info["sampled"]])
    return far, gap


@functools.lru_cache(maxsize=None)
def label_frames():
    """T = 3 frames of 2 - 4 lanes in the tiny geometry whose warped samples keep LABEL_MARGIN under every label set."""
    g = C.geometry("tiny")
    H, W, S = g["img_h"], g["img_w"], g["S"]
    rng = np.random.default_rng(404)
    out = []
    for want in (2, 4, 3):
        lanes = []
        while len(lanes) < want:
            lane = _lane(rng, H, W)
            far, gap = label_margins(lane, H, W, S)
            if far >= LABEL_MARGIN and gap >= LABEL_MIN_DY:
                lanes.append(lane)
        out.append(lanes)
    return out


@functools.lru_cache(maxsize=None)
def expected_labels(name):
    """[T, R, 6+S] float32 and the infos per frame of a label set, by the restatement."""
    g = C.geometry("tiny")
    p = params("tiny", name).numpy()
    labs, infos = [], []
    for t, lanes in enumerate(label_frames()):
        lab, inf = encode_frame_aug(lanes, g["img_h"], g["img_w"], g["S"], g["R"], p["flip2"][t], p["fwd"][t])
        labs.append(lab); infos.append(inf)
    out = np.stack(labs)
    out.setflags(write=False)
    return out, infos


# ---- image and labels agree: a 3 x 3 white blob on an annotated point of a vertical lane
BLOB_XY = (130.0, 12.0)                       # far from the centre (79.5, 31.5): the two rotation signs put it 11 px apart
BLOB_LANE = [(130.0, float(y)) for y in (60, 50, 40, 30, 20, 12, 2)]
BLOB_BOUND = 0.5                              # px: the quantisation of a 1/32-pixel tap grid plus the rounding of a 3 x 3 blob


def blob_frames():
    T, H, W = SHAPES["tiny"]
    f = np.zeros((T, H, W, 3), np.uint8)
    x, y = int(BLOB_XY[0]), int(BLOB_XY[1])
    f[:, y - 1:y + 2, x - 1:x + 2] = 255
    return f


def centroid(img):
    """Intensity centroid (x, y) of one image [H, W, 3]."""
    w = img.astype(np.float64).sum(axis=2)
    ys, xs = np.meshgrid(np.arange(img.shape[0]), np.arange(img.shape[1]), indexing="ij")
    return float((w * xs).sum() / w.sum()), float((w * ys).sum() / w.sum())


def lane_x_at(label_row, y, img_h, S):
    """x of an encoded lane (one valid row [6+S] without outside samples in front) at height y, by linear interpolation between the two
    sample rows around y."""
    ys = C.offsets(img_h, S)
    n_out, n_in = int(round(float(label_row[2]) * (S - 1))), int(round(float(label_row[5]) * (S - 1)))
    xs = label_row[6 + n_out:6 + n_out + n_in].astype(np.float64)
    rows = ys[n_out:n_out + n_in]                                                     # descending
    k = int(np.searchsorted(-rows, -y))                                               # rows[k-1] >= y > rows[k]
    assert 1 <= k < n_in, (k, n_in)
    a = (rows[k - 1] - y) / (rows[k - 1] - rows[k])
    return float(xs[k - 1] + a * (xs[k] - xs[k - 1]))
