"""Line clipping in the training targets (csrc/lane_targets.hip rule 0c, phnet_lane_targets_clip): a restatement of the rule of
include/phnet_hip.h in Python doubles, operation for operation, and the cases.

`clip_lane` cuts the MAPPED points of one lane (rules 0 / 0b already applied) at the rectangle and returns its fragments;
`encode_frame_clipped` maps, clips and feeds the fragments to tests/target_cases.py's `encode_lane` through its `encode_frame`, both
imported, not copied (the mapping is tests/augment_cases.py's `map_points`).  PARITY UNPINNED against imgaug / shapely: this file restates
the project's own rule.

Shapes: the three geometries of target_cases, Lin = 8, P = 64.  Every annotation coordinate is a multiple of 1/64.  The hand cases run
under the identity matrix, so their mapped points are their float32 inputs exactly and a point ON a bound is on it for the kernel too;
the random cases run under random 'basic' affines and keep `MARGIN` px between every mapped point and every bound, and C.MARGIN_X
between every sampled x and 0 / img_w (`guard`), so no last-bit difference can flip a predicate."""
import functools
import math
from unittest import mock

import numpy as np

from phnet_amd.libs.dataset.openlane.augment import AugmentParams
from tests import augment_cases as AC
from tests import target_cases as C

INSET = 1e-3                                  # Wc = img_w - INSET, Hc = img_h - INSET
LIN, PMAX = 8, 64                             # the padding of every case
MARGIN = 1e-3                                 # every mapped point of a guarded lane is at least this far from 0, Wc (x) and 0, Hc (y)
MIN_DY = 0.25                                 # adjacent points (in y) of a surviving fragment of a guarded lane are at least this far apart
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


# ------------------------------------------------------------------------------------------------------------ the restatement
def rect(img_h, img_w):
    return float(img_w) - INSET, float(img_h) - INSET


def is_in(p, Wc, Hc):
    return 0.0 <= p[0] <= Wc and 0.0 <= p[1] <= Hc                                   # False for NaN


def crossing(q, o, Wc, Hc):
    """From the in point q towards the out point o -> ((x, y), kept, (use_x, use_y)); kept False: it equals q and is dropped."""
    vx, vy = o[0] < 0.0 or o[0] > Wc, o[1] < 0.0 or o[1] > Hc
    bx, by = (0.0 if o[0] < 0.0 else Wc), (0.0 if o[1] < 0.0 else Hc)
    tx = (bx - q[0]) / (o[0] - q[0]) if vx else None
    ty = (by - q[1]) / (o[1] - q[1]) if vy else None
    use_x = vx and (not vy or tx <= ty)
    use_y = vy and (not vx or ty <= tx)
    t = tx if use_x else ty
    x, y = q[0] + t * (o[0] - q[0]), q[1] + t * (o[1] - q[1])
    x, y = (bx if use_x else x), (by if use_y else y)
    return (x, y), not (x == q[0] and y == q[1]), (use_x, use_y)


def clip_runs(points, img_h, img_w):
    """Rule 0c on the mapped points [(x, y)] of one lane -> [dict(a, b, E, X, points)], one per maximal run of in-points, in order;
    E / X: the crossing in front / behind, or None (absent or dropped).  A non-finite lane: one run, all its points."""
    pts = [(float(x), float(y)) for x, y in points]
    n = len(pts)
    if not all(math.isfinite(x) and math.isfinite(y) for x, y in pts):
        return [dict(a=0, b=n - 1, E=None, X=None, points=list(pts))]
    Wc, Hc = rect(img_h, img_w)
    inside = [is_in(p, Wc, Hc) for p in pts]
    runs, i = [], 0
    while i < n:
        if not inside[i]:
            i += 1
            continue
        a = i
        while i + 1 < n and inside[i + 1]:
            i += 1
        b = i
        E = X = None
        if a > 0:
            c, kept, _ = crossing(pts[a], pts[a - 1], Wc, Hc)
            E = c if kept else None
        if b < n - 1:
            c, kept, _ = crossing(pts[b], pts[b + 1], Wc, Hc)
            X = c if kept else None
        runs.append(dict(a=a, b=b, E=E, X=X, points=([E] if E else []) + pts[a:b + 1] + ([X] if X else [])))
        i += 1
    return runs


def clip_lane(points, img_h, img_w):
    """The fragments of one lane of mapped points, each a list of (x, y) doubles (rule 1 has not looked at them yet)."""
    return [r["points"] for r in clip_runs(points, img_h, img_w)]


def encode_frame_clipped(lanes, img_h, img_w, S, R, flip2=0, fwd=None, mapping=None, clip=True):
    """One frame -> (label float32 [R, 6+S], infos, frag_count): rules 0 / 0b, rule 0c when `clip`, then target_cases.encode_frame on the
    fragments (its `len > 2` filter is rule 1 on fragments).  frag_count: the surviving fragments before the R cap."""
    frags = []
    for lane in lanes:
        if len(lane) == 0:
            continue
        mapped = AC.map_points(lane, mapping, flip2, fwd, img_w)
        frags += clip_lane(mapped, img_h, img_w) if clip else [mapped]
    plain = C.encode_lane

    def lane_of_doubles(points, h, w, ys, _mapping=None):
        with mock.patch.object(C, "np", AC._NumpyWithoutTheCast()):
            return plain(points, h, w, ys, None)

    with mock.patch.object(C, "encode_lane", lane_of_doubles):
        label, infos = C.encode_frame(frags, img_h, img_w, S, R, mapping=None)
    return label, infos, sum(len(f) > 2 for f in frags)


# ---------------------------------------------------------------------------------------------------------------- the cases
def _hand(H, W):
    """Written for 320 x 800 and scaled with the image; what each is for is asserted in tests/test_lane_clip_cpu.py."""
    fy, fx = H / 320.0, W / 800.0
    q = C._q
    c = lambda xb, sl, bd, yb, yt, n: C.curve(xb * fx, sl * fx, bd * fx, yb * fy, yt * fy, n)        # noqa: E731
    s = lambda pts: [(q(x * fx), q(y * fy)) for x, y in pts]                                        # noqa: E731
    cases = []
    add = lambda name, lanes: cases.append(dict(name=name, lanes=lanes, spec={}))                   # noqa: E731
    add("all_in", [c(200, 80, 10, 310, 40, 7), c(600, -80, -10, 310, 40, 8)])
    add("all_out", [s([(-50, 300), (-40, 200), (-30, 100), (-20, 50)]), c(400, 50, 0, 300, 40, 6)])
    # left, right, top (y < 0), bottom (y > Hc: the lane starts below the image, so its fragment starts with E)
    add("four_edges", [c(100, -310, 0, 310, 40, 10), c(700, 300, 0, 310, 40, 10), c(400, 50, 0, 300, -60, 10), c(300, 100, 0, 380, 40, 10)])
    add("corner_tie", [[(24.0, 24.0), (16.0, 16.0), (8.0, 8.0), (-8.0, -8.0), (-16.0, -16.0)]])          # t_x = t_y = 1/2 exactly
    u = np.linspace(0.0, 1.0, 15)
    add("out_and_back", [[(q((700 + 200 * math.sin(math.pi * a)) * fx), q((310 - 280 * a) * fy)) for a in u], c(300, 60, 10, 305, 35, 9)])
    add("single_in_point", [s([(-10, 100), (20, 90), (-10, 80)])])
    add("run_of_one_at_start", [s([(20, 300), (-30, 250), (-40, 200), (-50, 150)]), c(500, 20, 5, 300, 50, 5)])
    add("both_out_across", [[(-10.0, q(50 * fy)), (W + 10.0, q(40 * fy)), (W + 20.0, q(30 * fy))]])
    add("border_t0", [[(q(40 * fx), q(120 * fy)), (q(20 * fx), q(110 * fy)), (0.0, q(100 * fy)), (-10.0, q(90 * fy))],
                      [(q(300 * fx), q(40 * fy)), (q(310 * fx), q(20 * fy)), (q(320 * fx), 0.0), (q(330 * fx), -20.0)]])
    add("nonfinite", [[(-50.0, q(300 * fy)), (float("nan"), q(200 * fy)), (q(100 * fx), q(100 * fy)), (q(120 * fx), q(50 * fy))],
                      c(600, -50, 0, 300, 40, 5)])
    zig = [((860, 700, 740)[k % 3], 300 - 15 * k) for k in range(19)]                # out, in, in, out, ...: six runs of two
    add("more_than_R", [s(zig)])
    return cases


def mapped_lane(lane, spec_row, img_w):
    """The lane's points behind rule 0b of a table row (flip2, fwd)."""
    return AC.map_points(lane, None, spec_row[0], spec_row[1], img_w)


def guard(lane, spec_row, H, W, ys):
    """The `_acceptable` idea of target_cases for a lane behind a matrix: (least distance of a mapped coordinate to a bound of the
    rectangle, least y gap of adjacent points of a surviving fragment, least distance of a sampled x to 0 / img_w)."""
    Wc, Hc = rect(H, W)
    pts = mapped_lane(lane, spec_row, W)
    far = min(min(abs(x), abs(x - Wc), abs(y), abs(y - Hc)) for x, y in pts)
    gap = edge = np.inf
    for frag in clip_lane(pts, H, W):
        if len(frag) <= 2:
            continue
        sy = sorted(y for _, y in frag)
        gap = min(gap, min(b - a for a, b in zip(sy[:-1], sy[1:])))
        with mock.patch.object(C, "np", AC._NumpyWithoutTheCast()):
            _, info = C.encode_lane(frag, H, W, ys, None)
        edge = min([edge] + [min(abs(x), abs(x - W)) for x in info["sampled"]])
    return far, gap, edge


def guarded(lane, spec_row, H, W, ys):
    far, gap, edge = guard(lane, spec_row, H, W, ys)
    return far >= MARGIN and gap >= MIN_DY and edge >= C.MARGIN_X


RANDOM_FRAMES = {"main": 12, "fine": 8, "tiny": 8}
SEEDS = {"main": 1101, "fine": 1202, "tiny": 1303}
# both ends of the 'basic' ranges (transforms.py:190-249), behind the second flip
ENDS = (dict(flip=True, rotate=-10.0, scale=0.8, translate=(-0.1, -0.1)), dict(flip=True, rotate=10.0, scale=1.2, translate=(0.1, 0.1)),
        dict(flip=False, rotate=10.0, scale=0.8, translate=(0.1, -0.1)), dict(flip=True, rotate=-10.0, scale=1.2, translate=(-0.1, 0.1)))


def _table_row(spec, H, W):
    p = AugmentParams.build([spec], H, W).numpy()
    return int(p["flip2"][0]), [float(v) for v in p["fwd"][0]]


def _random_lane(rng, H, W):
    """target_cases' random lane, or (one in two) one that weaves across the left or the right border: several runs."""
    if rng.random() >= 0.5:
        return C._random_lane(rng, H, W)[:PMAX]
    n = int(rng.integers(8, 40))
    ys = np.linspace(H * rng.uniform(0.7, 1.0), H * rng.uniform(0.0, 0.25), n)
    side = W * (0.0 if rng.random() < 0.5 else 1.0)
    x = side + W * rng.uniform(0.03, 0.12) * np.sin(np.arange(n) * rng.uniform(0.3, 1.2) + rng.uniform(0, 6)) + W * rng.uniform(-0.03, 0.03)
    return [(C._q(a), C._q(b)) for a, b in zip(x, ys)]


@functools.lru_cache(maxsize=None)
def cases(name):
    """[dict(name, lanes, spec[, random])] of one geometry: the hand cases under the identity, random frames whose lanes stay inside
    (identity), random frames under random 'basic' draws, and random frames under the ends of the 'basic' ranges."""
    g = C.geometry(name)
    H, W, S = g["img_h"], g["img_w"], g["S"]
    ys = C.offsets(H, S)
    out = _hand(H, W)
    rng = np.random.default_rng(SEEDS[name])
    Wc, Hc = rect(H, W)

    def frame(label, spec, all_in=False):
        row = _table_row(spec, H, W)
        lanes, want = [], int(rng.integers(1, 6))
        while len(lanes) < want:
            lane = _random_lane(rng, H, W)
            if all_in and not all(is_in(p, Wc, Hc) for p in mapped_lane(lane, row, W)):
                continue
            if guarded(lane, row, H, W, ys):
                lanes.append(lane)
        out.append(dict(name=label, lanes=lanes, spec=spec, random=True))

    for k in range(2):
        frame(f"inside_{k}", {}, all_in=True)
    for k in range(RANDOM_FRAMES[name]):
        spec = dict(flip=bool(rng.random() < 0.5), rotate=float(rng.uniform(-10, 10)), scale=float(rng.uniform(0.8, 1.2)),
                    translate=(float(rng.uniform(-0.1, 0.1)), float(rng.uniform(-0.1, 0.1))))
        frame(f"random_{k}", spec)
    for k, spec in enumerate(ENDS):
        frame(f"ends_{k}", spec)
    return out


@functools.lru_cache(maxsize=None)
def params(name):
    """The AugmentParams (host) of the geometry's cases, one row per frame."""
    g = C.geometry(name)
    return AugmentParams.build([c["spec"] for c in cases(name)], g["img_h"], g["img_w"])


def table_rows(name):
    p = params(name).numpy()
    return [(int(a), [float(v) for v in b]) for a, b in zip(p["flip2"], p["fwd"])]


@functools.lru_cache(maxsize=None)
def expected(name, clip=True):
    """[(label float32 [R, 6+S], infos, frag_count)] per case of the geometry, by the restatement; read-only."""
    g = C.geometry(name)
    out = []
    for c, (flip2, fwd) in zip(cases(name), table_rows(name)):
        label, infos, n = encode_frame_clipped(c["lanes"], g["img_h"], g["img_w"], g["S"], g["R"], flip2, fwd, clip=clip)
        label.setflags(write=False)
        out.append((label, infos, n))
    return out


def case(name, case_name):
    i = [c["name"] for c in cases(name)].index(case_name)
    return (cases(name)[i],) + expected(name)[i]


def packed(name):
    return C.pack([c["lanes"] for c in cases(name)], LIN, PMAX)


# ---- more than one ballot per lane: 254 points (the limit with rule 0c) that weave across the right border, so that runs start in one
# group of 64 points and end in the next, and a short lane behind it whose row number depends on all of them
LONG = dict(img_h=320, img_w=800, S=36, R=8, lin=2, pmax=254)


@functools.lru_cache(maxsize=None)
def long_case():
    """(lanes, (label [8, 6+36], infos, frag_count)) under the identity map: the weaving lane gives six fragments, the seventh row is
    the short lane's."""
    n = LONG["pmax"]
    weave = [(C._q(700.0 + 150.0 * math.sin(2.0 * math.pi * i / 50.0)), C._q(318.0 - 310.0 * i / (n - 1))) for i in range(n)]
    lanes = [weave, C.curve(300, 60, 10, 305, 35, 9)]
    want = encode_frame_clipped(lanes, LONG["img_h"], LONG["img_w"], LONG["S"], LONG["R"], 0, list(IDENTITY))
    want[0].setflags(write=False)
    return lanes, want
