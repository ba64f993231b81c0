"""Training targets (csrc/lane_targets.hip): a restatement of the rules in include/phnet_hip.h in Python doubles, and the cases.

The restatement follows the reference's libs/dataset/openlane/transforms.py (transform_annotation, filter_lane, sample_lane) rule
by rule, with ONE substitution: where the reference builds scipy's InterpolatedUnivariateSpline(k = min(3, n - 1)) it solves the
same interpolant explicitly - the line (n = 2), the parabola in Newton form (n = 3), the not-a-knot cubic spline by a tridiagonal
solve for the knot derivatives (n >= 4) - which is the kernel's algorithm, operation for operation.  Python floats are IEEE
doubles and nothing here is contracted, so the kernel can be held to it closely; tests/golden/targets_tiny.json holds what the
reference's own code gives on the same cases (tests/golden/make_goldens_targets.py).

Every coordinate of every case is a multiple of 1/64 (float32-representable, short in JSON).  `info` records which branch each
row took, so tests/test_targets_cpu.py can show without a GPU that the hand cases reach what they are for."""
import functools
import math
import os

import numpy as np

INVALID = -1e5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "targets_tiny.json")
EXACT = (0, 1, 2, 5)                          # flags, start and length: compared exactly
LIN, PMAX = 8, 256                            # the padding of every case: lanes per frame, points per lane
Q = 64.0                                      # coordinates are integers / Q

# (name, img_h, img_w, S, R).  np.arange(img_h, -1, -img_h / (S - 1)) has exactly S entries for each (asserted in offsets()).
GEOMETRIES = (("main", 320, 800, 36, 4), ("fine", 384, 768, 72, 4), ("tiny", 64, 160, 36, 4))


def geometry(name):
    return dict(zip(("name", "img_h", "img_w", "S", "R"), next(g for g in GEOMETRIES if g[0] == name)))


def offsets(img_h, S):
    """The reference's cfg.offsets_ys, as numpy builds it (its last entry is not exactly 0)."""
    ys = np.arange(img_h, -1, -(img_h / (S - 1)))
    if len(ys) != S:
        raise ValueError(f"np.arange({img_h}, -1, -{img_h}/{S - 1}) has {len(ys)} entries, not {S}")
    return ys


# ------------------------------------------------------------------------------------------------------------ the restatement
def lane_map(crop, src_w, scale_x, scale_y, flip):
    return dict(crop=float(crop), src_w=float(src_w), scale_x=float(scale_x), scale_y=float(scale_y), flip=bool(flip))


def map_for(out_h, out_w, src_h, src_w, crop, flip=False):
    """datasetOL.cropping, then the resize rule of DESIGN.md (each ratio formed once, in double)."""
    return lane_map(crop, src_w, float(out_w) / float(src_w), float(out_h) / float(src_h - crop), flip)


def knot_derivatives(t, v):
    """First derivatives of the not-a-knot cubic spline through (t[i], v[i]), t ascending, n >= 4: the tridiagonal system
         h1 s0 + (h0 + h1) s1                            = ((h0 + 2 D0) h1 m0 + h0^2 m1) / D0,          D0 = t2 - t0
         h_i s_(i-1) + 2 (h_(i-1) + h_i) s_i + h_(i-1) s_(i+1) = 3 (h_i m_(i-1) + h_(i-1) m_i),         i = 1 .. n-2
         D1 s_(n-2) + h_(n-3) s_(n-1)                    = (h_(n-2)^2 m_(n-3) + (2 D1 + h_(n-2)) h_(n-3) m_(n-2)) / D1,   D1 = t_(n-1) - t_(n-3)
    (h_i = t_(i+1) - t_i, m_i = (v_(i+1) - v_i) / h_i) by forward elimination without pivoting and back substitution."""
    n = len(t)
    h = lambda i: t[i + 1] - t[i]
    m = lambda i: (v[i + 1] - v[i]) / (t[i + 1] - t[i])
    cp, dp = [0.0] * n, [0.0] * n
    d0 = t[2] - t[0]
    b = h(1)
    cp[0] = d0 / b
    dp[0] = (((h(0) + 2.0 * d0) * h(1)) * m(0) + (h(0) * h(0)) * m(1)) / d0 / b
    for i in range(1, n - 1):
        a = h(i)
        den = 2.0 * (h(i - 1) + h(i)) - a * cp[i - 1]
        cp[i] = h(i - 1) / den
        dp[i] = (3.0 * (h(i) * m(i - 1) + h(i - 1) * m(i)) - a * dp[i - 1]) / den
    d1 = t[n - 1] - t[n - 3]
    den = h(n - 3) - d1 * cp[n - 2]
    rhs = ((h(n - 2) * h(n - 2)) * m(n - 3) + ((2.0 * d1 + h(n - 2)) * h(n - 3)) * m(n - 2)) / d1
    s = [0.0] * n
    s[n - 1] = (rhs - d1 * dp[n - 2]) / den
    for i in range(n - 2, -1, -1):
        s[i] = dp[i] - cp[i] * s[i + 1]
    return s


def interpolate(t, v, s, y):
    """The interpolant of rule 4 at y, t[0] <= y <= t[-1]."""
    n = len(t)
    if n == 2:
        return v[0] + (y - t[0]) * ((v[1] - v[0]) / (t[1] - t[0]))
    if n == 3:
        d01 = (v[1] - v[0]) / (t[1] - t[0])
        d12 = (v[2] - v[1]) / (t[2] - t[1])
        d012 = (d12 - d01) / (t[2] - t[0])
        return v[0] + (y - t[0]) * (d01 + (y - t[1]) * d012)
    lo, hi = 0, n - 2                                  # the last i with t[i] <= y, at most n - 2
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if t[mid] <= y:
            lo = mid
        else:
            hi = mid - 1
    i = lo
    h = t[i + 1] - t[i]
    m = (v[i + 1] - v[i]) / h
    tt = (s[i] + s[i + 1] - 2.0 * m) / h
    c0 = tt / h
    c1 = (m - s[i]) / h - tt
    d = y - t[i]
    return ((c0 * d + c1) * d + s[i]) * d + v[i]


def encode_lane(points, img_h, img_w, ys, mapping=None):
    """One surviving lane (points: [(x, y)], float32 values) -> (row values or None, info).  row values = dict(n_out, n_in, xs:
    the reordered doubles, theta).  info: what happened."""
    S = len(ys)
    strip = float(img_h) / (S - 1)
    info = dict(status="valid", n=0, n_ext=0, n_interp=0, n_out=0, n_in=0, reordered=False, negative_thetas=0, sampled=[])
    pts = [(float(np.float32(x)), float(np.float32(y))) for x, y in points]
    if mapping is not None:
        mp = []
        for x, y in pts:
            y = y - mapping["crop"]
            if mapping["flip"]:
                x = (mapping["src_w"] - 1.0) - x
            mp.append((x * mapping["scale_x"], y * mapping["scale_y"]))
        pts = mp
    if not all(math.isfinite(x) and math.isfinite(y) for x, y in pts):
        info["status"] = "nonfinite"
        return None, info
    order = sorted(range(len(pts)), key=lambda i: -pts[i][1])                     # stable
    seen, kept = set(), []
    for i in order:
        if pts[i][1] not in seen:
            seen.add(pts[i][1])
            kept.append(pts[i])
    kept = [(x * float(img_w) / float(img_w), y * float(img_h) / float(img_h)) for x, y in kept]
    n = info["n"] = len(kept)
    if n < 2:
        info["status"] = "one_point"
        return None, info
    t = [p[1] for p in reversed(kept)]                                            # ascending y
    v = [p[0] for p in reversed(kept)]
    y_min, y_max = t[0], t[n - 1]
    s = knot_derivatives(t, v) if n >= 4 else None
    slope = (v[n - 1] - v[n - 2]) / (t[n - 1] - t[n - 2])                       # the two bottom-most points
    ext, inter = [], []
    for y in (float(u) for u in ys):
        if y > y_max:
            ext.append(v[n - 1] + (y - t[n - 1]) * slope)
        elif y >= y_min:
            inter.append(interpolate(t, v, s, y))
    info["n_ext"], info["n_interp"] = len(ext), len(inter)
    if not inter:
        info["status"] = "no_row"
        return None, info
    all_xs = ext + inter
    info["sampled"] = all_xs
    inside = [0.0 <= x < float(img_w) for x in all_xs]
    xs_out = [x for x, k in zip(all_xs, inside) if not k]
    xs_in = [x for x, k in zip(all_xs, inside) if k]
    info["n_out"], info["n_in"] = len(xs_out), len(xs_in)
    info["reordered"] = any((not k) and any(inside[:j]) for j, k in enumerate(inside))
    if len(xs_in) <= 1:
        info["status"] = "few_inside"
        return None, info
    total = 0.0
    for i in range(1, len(xs_in)):
        th = math.atan(i * strip / (xs_in[i] - xs_in[0] + 1e-5)) / math.pi
        if not th > 0:
            th = 1 - abs(th)
            info["negative_thetas"] += 1
        total = total + th
    return dict(n_out=len(xs_out), n_in=len(xs_in), xs=xs_out + xs_in, theta=total / (len(xs_in) - 1)), info


def encode_frame(lanes, img_h, img_w, S, R, mapping=None, ys=None):
    """lanes: the annotation of one frame, a list of point lists -> (label float32 [R, 6+S], [info per consumed row])."""
    ys = offsets(img_h, S) if ys is None else ys
    label = np.full((R, 6 + S), INVALID, dtype=np.float32)
    label[:, 0], label[:, 1] = 1, 0
    infos = []
    survivors = [lane for lane in lanes if len(lane) > 2]
    for r, lane in enumerate(survivors[:R]):
        row, info = encode_lane(lane, img_h, img_w, ys, mapping)
        infos.append(info)
        if row is None:
            continue
        with np.errstate(over="ignore"):
            label[r, 0], label[r, 1] = 0, 1
            label[r, 2] = row["n_out"] / (S - 1)
            label[r, 3] = row["xs"][row["n_out"]] / (img_w - 1)
            label[r, 4] = row["theta"]
            label[r, 5] = row["n_in"] / (S - 1)
            label[r, 6:6 + len(row["xs"])] = row["xs"]
    return label, infos


def pack(frames, lin=LIN, pmax=PMAX):
    """Frames (lists of lanes) -> points f32 [F, lin, pmax, 2], counts i32 [F, lin], lanes_num i32 [F], zero padded."""
    pts = np.zeros((len(frames), lin, pmax, 2), np.float32)
    cnt = np.zeros((len(frames), lin), np.int32)
    num = np.zeros((len(frames),), np.int32)
    for f, lanes in enumerate(frames):
        assert len(lanes) <= lin
        num[f] = len(lanes)
        for l, lane in enumerate(lanes):
            assert len(lane) <= pmax
            cnt[f, l] = len(lane)
            if len(lane):
                pts[f, l, :len(lane)] = np.asarray(lane, np.float64)
    return pts, cnt, num


# ---------------------------------------------------------------------------------------------------------------- the cases
def _q(v):
    return float(np.round(np.asarray(v, np.float64) * Q) / Q)


def curve(x_bottom, slope, bend, y_bottom, y_top, n):
    """n points from (x_bottom, y_bottom) up to y_top: x = x_bottom + slope u + bend u^2, u in [0, 1]; multiples of 1/64."""
    ys = np.linspace(y_bottom, y_top, n)
    u = (y_bottom - ys) / float(y_bottom - y_top)
    return [(_q(x_bottom + slope * a + bend * a * a), _q(y)) for a, y in zip(u, ys)]


def _hand_main(H, W):
    """Hand cases, written for 320 x 800 with S = 36 (strip 9.142857: sample rows at 320, 310.857, 301.714, ...) and scaled
    with the image for the other geometries where that keeps their meaning."""
    fy, fx = H / 320.0, W / 800.0
    c = lambda xb, sl, bd, yb, yt, n: curve(xb * fx, sl * fx, bd * fx, yb * fy, yt * fy, n)
    cases = []
    add = lambda name, lanes, **kw: cases.append(dict(name=name, lanes=lanes, reference=kw.get("reference", True)))
    add("counts_3_4_5_37", [c(150, 120, 30, 300, 40, 3), c(330, 40, -20, 310, 30, 4), c(480, -30, 25, 305, 20, 5), c(640, -90, -30, 315, 12, 37)])
    add("count_256", [c(400, 150, -60, 318, 8, 256)] if H >= 300 else [c(400, 150, -60, 318, 8, 40)])
    # two of three points share y: n = 2, the line.  Then three points on one y: n = 1, default row, row 1 is consumed
    add("dup_linear_and_one_y", [[(_q(200 * fx), _q(300 * fy)), (_q(260 * fx), _q(100 * fy)), (_q(700 * fx), _q(100 * fy))],
                                 [(_q(300 * fx), _q(150 * fy)), (_q(320 * fx), _q(150 * fy)), (_q(340 * fx), _q(150 * fy))],
                                 c(520, -60, 10, 300, 30, 6)])
    add("two_point_lane_between", [c(200, 80, 10, 310, 40, 7), [(_q(400 * fx), _q(300 * fy)), (_q(410 * fx), _q(100 * fy))], c(600, -80, -10, 310, 40, 8)])
    add("five_long", [c(100 + 140 * k, 60 - 30 * k, 8, 312, 24, 6 + k) for k in range(5)])
    lane = c(350, 90, -35, 308, 18, 12)
    perm = np.random.default_rng(3).permutation(len(lane))
    add("shuffled", [lane, [lane[i] for i in perm]])
    # duplicates of y with other x, after the first in input order: (x + 50) must lose wherever it stands
    base = c(420, -70, 20, 300, 36, 9)
    dup = [base[4], base[1], (base[1][0] + 50.0, base[1][1]), base[7], base[0], base[2], (base[4][0] - 50.0, base[4][1]), base[3], base[5], base[6], base[8],
           (base[8][0] + 50.0, base[8][1])]
    add("dup_first_wins", [dup, [base[i] for i in (4, 1, 7, 0, 2, 3, 5, 6, 8)]])
    add("between_rows", [[(_q(300 * fx), _q(312 * fy)), (_q(302 * fx), _q(314.5 * fy)), (_q(305 * fx), _q(318 * fy))], c(500, 20, 5, 300, 50, 5)])
    add("top_at_zero", [c(380, 60, -15, 300, 0, 11)])
    add("bottom_exit", [c(770, -200, 30, 200, 20, 8), c(30, 220, -30, 190, 30, 7)])
    add("curves_out_top", [c(300, -150, -260, 310, 10, 14), c(500, 120, 300, 300, 6, 13)])
    add("at_most_one_inside", [c(-400, 390, 25, 300, 14, 9), c(1300, -300, -205, 310, 5, 9)])
    add("x_zero", [[(0.0, _q(y)) for y in np.linspace(H, 0, 9)]])
    # x = img_w exactly is outside, and the rules give it exactly.  FITPACK's k >= 2 evaluation of constant data at img_w lands a
    # few 1e-13 BELOW it on some rows (a valid row by rounding noise), its k = 1 evaluation is exact: the pinned case has two
    # distinct y (the top point annotated twice), the nine-point one is held to the rules alone
    add("x_width", [[(float(W), float(H)), (float(W), 0.0), (float(W), 0.0)]])
    add("x_width_cubic", [[(float(W), _q(y)) for y in np.linspace(H, 0, 9)]], reference=False)
    add("lean_left", [c(600, -300, -40, 315, 25, 10)])
    add("vertical", [[(_q(400 * fx), _q(y)) for y in np.linspace(310 * fy, 20 * fy, 7)]])
    add("no_lanes", [])
    add("nonfinite", [c(200, 50, 0, 300, 40, 5), [(_q(300 * fx), _q(300 * fy)), (float("nan"), _q(200 * fy)), (_q(320 * fx), _q(100 * fy)), (_q(330 * fx), _q(50 * fy))],
                      [(_q(500 * fx), _q(300 * fy)), (_q(510 * fx), float("inf")), (_q(520 * fx), _q(100 * fy))], c(600, -50, 0, 300, 40, 5)], reference=False)
    return cases


def _two_lane_tiny():
    return dict(name="two_lanes", lanes=[curve(40, 25, 6, 62, 6, 8), curve(110, -30, -5, 60, 4, 10)], reference=True)


RANDOM_FRAMES = {"main": 10, "fine": 6, "tiny": 4}
MARGIN_X = 1e-3                               # every sampled x of a random lane is at least this far from 0 and img_w
MIN_DY = 1.0                                  # adjacent points of a random lane are at least this far apart in y


def _random_lane(rng, H, W):
    y_bottom = H * rng.uniform(0.6, 1.0)
    y_top = H * rng.uniform(0.0, 0.3)
    span = y_bottom - y_top
    n = min(int(rng.integers(3, 40)), int(span / 3.0))
    gaps = 1.1 + (span - 1.1 * (n - 1)) * rng.dirichlet(np.ones(n - 1))          # each >= 1.1: still >= MIN_DY in 1/64ths
    ys = y_bottom - np.concatenate([[0.0], np.cumsum(gaps)])
    u = (y_bottom - ys) / span
    x = W * rng.uniform(-0.1, 1.1) + W * rng.uniform(-0.6, 0.6) * u + W * rng.uniform(-0.3, 0.3) * u * u \
        + W * 0.01 * np.sin(u * rng.uniform(2, 9) + rng.uniform(0, 6))
    lane = [(_q(a), _q(b)) for a, b in zip(x, ys)]
    return [lane[i] for i in rng.permutation(n)] if rng.random() < 0.3 else lane


def _acceptable(lane, H, W, ys):
    pts = sorted(lane, key=lambda p: -p[1])
    if any(a[1] - b[1] < MIN_DY for a, b in zip(pts[:-1], pts[1:])):
        return False
    _, info = encode_lane(lane, H, W, ys)
    return all(min(abs(x), abs(x - W)) >= MARGIN_X for x in info["sampled"])


@functools.lru_cache(maxsize=None)
def cases(name):
    """[dict(name, lanes, reference)] of one geometry: the hand cases, then seeded random frames."""
    g = geometry(name)
    H, W, S = g["img_h"], g["img_w"], g["S"]
    ys = offsets(H, S)
    out = _hand_main(H, W) if name != "tiny" else [_two_lane_tiny()]
    rng = np.random.default_rng({"main": 101, "fine": 202, "tiny": 303}[name])
    for k in range(RANDOM_FRAMES[name]):
        lanes, want = [], int(rng.integers(1, 6))
        while len(lanes) < want:
            lane = _random_lane(rng, H, W)
            if _acceptable(lane, H, W, ys):
                lanes.append(lane)
        out.append(dict(name=f"random_{k}", lanes=lanes, reference=True, random=True))
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """[(label float32 [R, 6+S], infos)] per case of the geometry, by the restatement; read-only."""
    g = geometry(name)
    out = []
    for c in cases(name):
        label, infos = encode_frame(c["lanes"], g["img_h"], g["img_w"], g["S"], g["R"])
        label.setflags(write=False)
        out.append((label, infos))
    return out


def case(name, case_name):
    i = [c["name"] for c in cases(name)].index(case_name)
    return (cases(name)[i],) + expected(name)[i]


def source_frames(seed, n_frames, src_h=1280, src_w=1920, crop=480):
    """Annotations in camera coordinates (the map of rule 0 in front): smooth lanes below the sky crop, some points above it."""
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(n_frames):
        lanes = []
        for _ in range(int(rng.integers(1, 5))):
            n = int(rng.integers(3, 25))
            lanes.append(curve(src_w * rng.uniform(0.05, 0.95), src_w * rng.uniform(-0.5, 0.5), src_w * rng.uniform(-0.2, 0.2),
                               src_h * rng.uniform(0.85, 1.0), crop * rng.uniform(0.9, 1.4), n))
        frames.append(lanes)
    return frames


def ulps(a, b):
    """Distance in float32 ulps between two float32 arrays of finite values, elementwise (int64)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def golden_label(rec, R, S):
    lab = np.full((R, 6 + S), INVALID, np.float32)
    for r, row in enumerate(rec["label"]):
        lab[r, :len(row)] = row
    return lab


def assert_rows_match(got, want, max_ulps, what):
    """The comparison of the issue: exact fields exact, the -1e5 pattern exact, float fields within max_ulps float32 ulps."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    assert np.array_equal(got == INVALID, want == INVALID), (what, "positions of -1e5")
    assert np.array_equal(got[..., EXACT], want[..., EXACT]), (what, "flags / start / length")
    d = ulps(got, want)
    assert int(d.max()) <= max_ulps, (what, int(d.max()))
    return int(d.max())
