"""Lane overlay  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE: a numpy restatement of rules 1-5 of phnet_lane_draw
(include/phnet_hip.h) and the inputs tests/test_overlay_cpu.py and tests/test_overlay_gpu.py share.

`draw_reference` paints lane after lane in ascending packed index, the reference's loop (testOL.py:174-177), so the last lane
painted wins - the order rule without any reference to how the kernel finds it.  Everything is int64 / float64 numpy."""
import numpy as np

COORD_BOUND = 8192                     # rule 1: a pixel coordinate outside [-8192, 8192] drops the point


def map_points(xy, sx, sy, oy):
    """Rule 1 on xy f32 [n,2] -> int64 [m,2] pixel points of the survivors, in order."""
    xy = np.asarray(xy, dtype=np.float32)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        fx = x * np.float64(sx)
        fy = y * np.float64(sy) + np.float64(oy)
        ok = (x > 0) & (y > 0) & np.isfinite(fx) & np.isfinite(fy)
        tx, ty = np.trunc(np.where(ok, fx, 0.0)), np.trunc(np.where(ok, fy, 0.0))
    ok &= (np.abs(tx) <= COORD_BOUND) & (np.abs(ty) <= COORD_BOUND)
    return np.stack([tx[ok], ty[ok]], axis=1).astype(np.int64)


def cover(pix, height, width, lane_width):
    """Rule 2: bool [height,width], the pixels within lane_width / 2 of the polyline through pix int64 [m,2] (m < 2: none)."""
    mask = np.zeros((height, width), dtype=bool)
    w2 = np.int64(lane_width) * np.int64(lane_width)
    reach = (lane_width + 1) // 2                    # no pixel further than this from a segment's box is within lane_width / 2 of it
    for (x0, y0), (x1, y1) in zip(pix[:-1], pix[1:]):
        xa, xb = max(0, min(x0, x1) - reach), min(width - 1, max(x0, x1) + reach)
        ya, yb = max(0, min(y0, y1) - reach), min(height - 1, max(y0, y1) + reach)
        if xa > xb or ya > yb:
            continue
        v, u = np.mgrid[ya:yb + 1, xa:xb + 1].astype(np.int64)
        dx, dy = np.int64(x1 - x0), np.int64(y1 - y0)
        qx, qy = u - x0, v - y0
        dot, L2 = qx * dx + qy * dy, dx * dx + dy * dy
        before = 4 * (qx * qx + qy * qy) <= w2
        past = 4 * ((u - x1) ** 2 + (v - y1) ** 2) <= w2
        cross = qx * dy - qy * dx
        between = 4 * cross * cross <= w2 * L2
        mask[ya:yb + 1, xa:xb + 1] |= np.where(dot <= 0, before, np.where(dot >= L2, past, between))
    return mask


def lane_value(k, slot=None, track_id=None):
    """Rule 4 for packed lane k of one frame (slot, track_id: that frame's int32 [L] rows, or None)."""
    if track_id is None:
        return k + 1
    s = int(slot[k])
    ident = int(track_id[s]) if 0 <= s < len(track_id) else 0
    return 1 + (ident - 1) % 254 if ident >= 1 else 255


def draw_reference(points, count, lanes_num, out_hw, sx, sy, oy, lane_width, slot=None, track_id=None, src_rgb=None, palette=None,
                   alpha=256):
    """points f32 [F,L,S,2], count i32 [F,L], lanes_num i32 [F] (numpy) -> dict(label_map u8 [F,H,W], overlay u8 [F,H,W,3]).
    src_rgb: the source ALREADY converted to 8-bit RGB, u8 [F,H,W,3] (None: black); the overlay needs `palette` u8 [256,3]."""
    points, count, lanes_num = np.asarray(points), np.asarray(count), np.asarray(lanes_num)
    F, L, S = points.shape[:3]
    H, W = out_hw
    label = np.zeros((F, H, W), dtype=np.uint8)
    for f in range(F):
        for k in range(min(max(int(lanes_num[f]), 0), L)):                       # ascending: a later lane paints over an earlier one
            c = min(max(int(count[f, k]), 0), S)
            pix = map_points(points[f, k, :c], sx, sy, oy)
            if len(pix) < 2:
                continue
            v = lane_value(k, None if slot is None else slot[f], None if track_id is None else track_id[f])
            label[f][cover(pix, H, W, lane_width)] = v
    out = dict(label_map=label, overlay=None)
    if palette is not None:
        src = np.zeros((F, H, W, 3), dtype=np.int64) if src_rgb is None else np.asarray(src_rgb).astype(np.int64)
        pal = np.asarray(palette).astype(np.int64)[label]                        # [F,H,W,3]
        mixed = (src * (256 - alpha) + pal * alpha + 128) >> 8
        out["overlay"] = np.where((label > 0)[..., None], mixed, src).astype(np.uint8)
    return out


def source_rgb(fmt, surfaces, H, W, pitch, surface_rows, csc):
    """Rule 5's source pixel, restated the way the kernel folds it: c = clip((bias + m0 Y + m1 U + m2 V) >> 20, 0, 255) with
    bias = 2^19 - m0 y0 - 128 (m1 + m2), chroma replicated.  surfaces u8 [F, *frame_shape] -> u8 [F,H,W,3]."""
    s = np.asarray(surfaces)
    if fmt == "rgb":
        return s.reshape(s.shape[0], H, W, 3)
    r, x = np.arange(H)[:, None], np.arange(W)[None, :]
    if fmt == "nv12":
        Y, U, V = s[:, r, x], s[:, surface_rows + r // 2, 2 * (x // 2)], s[:, surface_rows + r // 2, 2 * (x // 2) + 1]
    else:
        Y, U, V = s[:, r, 2 * x], s[:, r, 4 * (x // 2) + 1], s[:, r, 4 * (x // 2) + 3]
    Y, U, V = (a.astype(np.int64) for a in (Y, U, V))
    csc = np.asarray(csc, dtype=np.int64)
    m = csc[1:].reshape(3, 3)
    out = [np.clip(((1 << 19) - m[c, 0] * csc[0] - 128 * (m[c, 1] + m[c, 2]) + m[c, 0] * Y + m[c, 1] * U + m[c, 2] * V) >> 20, 0, 255)
           for c in range(3)]
    return np.stack(out, axis=-1).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------------ inputs
def random_lanes(F, L, S, seed, reach=1.0):
    """Seeded polylines laid out as phnet_lane_points lays them out: points f32 [F,L,S,2] (random walks that start anywhere in
    the image, wander out of it on the right, at the bottom and - with oy < 0 - at the top, and come back; a few points are
    x <= 0, NaN, +-inf or 1e30; some consecutive points are identical), count i32 [F,L] from 0 to S, lanes_num i32 [F] from 0 to
    L with both ends taken.  `reach` scales the step, so long segments occur."""
    g = np.random.default_rng(seed)
    start = g.uniform(0.02, 1.1, (F, L, 1, 2))
    steps = g.normal(0.0, 0.12 * reach, (F, L, S, 2))
    steps[g.random((F, L, S)) < 0.08] = 0.0                                      # identical consecutive points
    pts = (start + np.cumsum(steps, axis=2)).astype(np.float32)
    odd = g.random((F, L, S))
    pts[odd < 0.02, 0] = np.float32(-0.25)
    pts[(odd >= 0.02) & (odd < 0.03), 0] = 0.0
    pts[(odd >= 0.03) & (odd < 0.04), 1] = np.float32("nan")
    pts[(odd >= 0.04) & (odd < 0.05), 0] = np.float32("inf")
    pts[(odd >= 0.05) & (odd < 0.06), 1] = np.float32("-inf")
    pts[(odd >= 0.06) & (odd < 0.07), 0] = np.float32(1e30)
    pts[(odd >= 0.07) & (odd < 0.09)] *= np.float32(40.0)                        # end points far outside, some beyond the bound
    count = g.integers(0, S + 1, (F, L)).astype(np.int32)
    count[g.random((F, L)) < 0.5] = S
    lanes_num = g.integers(0, L + 1, (F,)).astype(np.int32)
    lanes_num[0], lanes_num[-1] = L, 0 if F > 1 else L
    return pts, count, lanes_num


def adversarial_frames(S=8):
    """Five literal frames of L = 4 lanes, S points each, in normalised coordinates for a renderer with sx = W, sy = H + 8, oy = -8
    (so y < 8 / (H + 8) is above the image):
      0  two lanes crossing, a third lying exactly on the first (the order rule decides every pixel of it), a fourth on part of the
         second;
      1  a lane that leaves the image on the right and comes back, one that leaves at the bottom and comes back, one at the top; a
         lane whose end points lie far outside on both ends (left exits cannot exist: rule 1 skips x <= 0);
      2  x <= 0, NaN, +-inf and 1e30 between good points (the survivors on both sides join), identical consecutive points, a lane
         that is one point repeated;
      3  lanes_num = 0 over points that would draw;
      4  lanes_num = L with counts 0, 1, 2 and S.
    -> points f32 [5,4,S,2], count i32 [5,4], lanes_num i32 [5]."""
    assert S >= 8
    nan, inf = float("nan"), float("inf")
    P = np.zeros((5, 4, S, 2), dtype=np.float32)
    count = np.zeros((5, 4), dtype=np.int32)

    def put(f, k, pts):
        P[f, k] = np.asarray((list(pts) + [pts[-1]] * S)[:S], dtype=np.float32)     # the tail beyond `count` repeats the last point

    diag = [(0.1 + 0.8 * i / 7, 0.25 + 0.7 * i / 7) for i in range(8)]
    anti = [(0.9 - 0.8 * i / 7, 0.25 + 0.7 * i / 7) for i in range(8)]
    put(0, 0, diag); put(0, 1, anti); put(0, 2, diag); put(0, 3, anti[2:6])
    count[0] = (8, 8, 8, 4)
    put(1, 0, [(0.6, 0.5), (0.9, 0.55), (1.4, 0.6), (1.5, 0.7), (0.95, 0.75), (0.5, 0.8)])
    put(1, 1, [(0.2, 0.7), (0.25, 0.95), (0.3, 1.3), (0.4, 1.35), (0.45, 0.9), (0.5, 0.6)])
    put(1, 2, [(0.7, 0.4), (0.72, 0.1), (0.75, 0.01), (0.8, 0.02), (0.82, 0.3)])
    put(1, 3, [(30.0, 20.0), (0.5, 0.5), (60.0, 0.3)])
    count[1] = (6, 6, 5, 3)
    put(2, 0, [(0.1, 0.9), (0.0, 0.8), (0.3, 0.7), (nan, 0.6), (0.5, 0.5), (0.6, -inf), (inf, 0.4), (0.8, 0.35)])
    put(2, 1, [(0.2, 0.3), (1e30, 0.3), (0.2, 0.3), (0.2, 0.3), (0.4, 0.3), (0.4, 0.3), (-0.5, 0.3), (0.6, 0.45)])
    put(2, 2, [(0.5, 0.8)] * 8)
    put(2, 3, [(0.9, 0.9), (0.9, nan), (nan, 0.9), (0.7, 0.0)])                  # one survivor only
    count[2] = (8, 8, 8, 4)
    for k in range(4):
        put(3, k, diag)
    count[3] = 8
    put(4, 0, diag); put(4, 1, anti); put(4, 2, [(0.5, 0.3), (0.5, 0.9)]); put(4, 3, [(0.3 + 0.05 * i, 0.5) for i in range(S)])
    count[4] = (0, 1, 2, S)
    return P, count, np.array([4, 4, 4, 0, 4], dtype=np.int32)
