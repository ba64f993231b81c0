"""Validation F1 on the device (csrc/lane_eval.hip): a numpy restatement of the rules of include/phnet_hip.h - presence, the wire
round trip, the spline, the end points, the matching and the counters - and the cases the CPU and the GPU tests share.  The
restatement is written from the rules, scalar by scalar where the order of operations matters; tests/test_f1_cpu.py holds it to
the host evaluator (phnet_amd/evaluation/culane.py, generate_lane.py), tests/test_f1_gpu.py holds the kernels to it."""
import math
from fractions import Fraction

import numpy as np

H, W, LANE_W, THRESHOLD = 96, 160, 5, 0.5                  # canvas and evaluator options
G, L, S, P = 3, 4, 8, 9
SIZE, CROP_TOP = (80, 160), 16                             # wire: x = tx * 80, y = ty * 40 + 8
TIMES, COORD, RELABEL_CAP = 50, 8192, 1024
C = (max(S, P) - 1) * TIMES
f64, f32 = np.float64, np.float32


# ------------------------------------------------------------------------------------------------ rules 1 and 2
def wire_value(v) -> np.float32:
    """The one-decimal text round trip of rule 2 on a double."""
    v = float(v)
    with np.errstate(all="ignore"):
        if v != v or math.isinf(v):
            return f32(v)
        q = v * 10.0
        k = float(np.rint(q))
        fl = math.floor(q)
        if q - fl == 0.5:
            r = Fraction(v) * 10 - Fraction(q)             # what fma(v, 10, -q) rounds: its sign is exact
            if r > 0:
                k = fl + 1.0
            elif r < 0:
                k = float(fl)
        return f32(k / 10.0)


def lane_of(t: dict, f: int, j: int, mode: str, size=SIZE, crop_top=CROP_TOP):
    """Lane j of image f of a table set -> (present, float32 [n,2] in evaluator coordinates)."""
    g_, l_ = t["gt_count"].shape[1], t["count"].shape[1]
    if j < g_:
        p_ = t["gt_points"].shape[2]
        n = min(max(int(t["gt_count"][f, j]), 0), p_)
        return j < min(max(int(t["gt_num"][f]), 0), g_), t["gt_points"][f, j, :n].astype(f32)
    k = j - g_
    s_ = t["points"].shape[2]
    n = min(max(int(t["count"][f, k]), 0), s_)
    present = k < min(max(int(t["lanes_num"][f]), 0), l_)
    pts = t["points"][f, k, :n].astype(f32)
    if mode == "raw":
        return present, pts
    out = np.zeros((n, 2), f32)
    for i in range(n):
        tx, ty = pts[n - 1 - i]
        with np.errstate(all="ignore"):
            out[i, 0] = wire_value((f64(tx) * f64(size[1])) / f64(2))
            out[i, 1] = wire_value((f64(ty) * f64(size[0]) + f64(crop_top)) / f64(2))
    return present and n > 2, out


# ------------------------------------------------------------------------------------------------ rules 3 and 4
def polyline(lane: np.ndarray) -> np.ndarray:
    """Rule 3: float32 [m,2] polyline of a lane of n >= 2 points (product-form cube, every operation a rounded double one)."""
    n = len(lane)
    if n == 2:
        return lane.astype(f32)
    p = lane.astype(f64)
    with np.errstate(all="ignore"):
        h = [np.sqrt((p[i + 1, 0] - p[i, 0]) * (p[i + 1, 0] - p[i, 0]) + (p[i + 1, 1] - p[i, 1]) * (p[i + 1, 1] - p[i, 1]))
             for i in range(n - 1)]
        out = np.zeros(((n - 1) * TIMES + 1, 2), f32)
        for a in range(2):
            d = [p[i + 1, a] - p[i, a] for i in range(n - 1)]
            cc = [h[i + 1] for i in range(n - 2)]
            dd = [f64(6) * (d[i + 1] / h[i + 1] - d[i] / h[i]) for i in range(n - 2)]
            b0 = f64(2) * (h[0] + h[1])
            cc[0] = cc[0] / b0
            dd[0] = dd[0] / b0
            for i in range(1, n - 2):
                tmp = f64(2) * (h[i] + h[i + 1]) - h[i] * cc[i - 1]
                cc[i] = cc[i] / tmp
                dd[i] = (dd[i] - h[i] * dd[i - 1]) / tmp
            m = [f64(0)] * n
            m[n - 2] = dd[n - 3]
            for i in range(n - 4, -1, -1):
                m[i + 1] = dd[i] - cc[i] * m[i + 2]
            m[0] = f64(0)
            m[n - 1] = f64(0)
            for i in range(n - 1):
                b = d[i] / h[i] - ((f64(2) * h[i]) * m[i] + h[i] * m[i + 1]) / f64(6)
                c = m[i] / f64(2)
                e = (m[i + 1] - m[i]) / (f64(6) * h[i])
                for k in range(TIMES):
                    t = (h[i] / f64(TIMES)) * f64(k)
                    t2 = t * t
                    out[i * TIMES + k, a] = f32(p[i, a] + b * t + c * t2 + e * (t2 * t))
            out[-1, a] = lane[-1, a]
    return out


def end_points(poly: np.ndarray) -> np.ndarray:
    """Rule 4: int32 [m,2]."""
    with np.errstate(all="ignore"):
        q = poly.astype(f64)
        q = np.where(q != q, 0.0, q)
        return np.minimum(np.maximum(np.rint(q), -COORD), COORD).astype(np.int32)


def segment_table(t: dict, mode: str, size=SIZE, crop_top=CROP_TOP):
    """-> (segs int32 [F*(G+L), C, 5], lane_pts int32 [F, G+L]) by rules 1-4."""
    f_, g_, l_ = t["gt_num"].shape[0], t["gt_count"].shape[1], t["count"].shape[1]
    c_ = (max(t["points"].shape[2], t["gt_points"].shape[2]) - 1) * TIMES
    segs = np.zeros((f_ * (g_ + l_), c_, 5), np.int32)
    segs[:, :, 4] = -1
    lane_pts = np.full((f_, g_ + l_), -1, np.int32)
    for f in range(f_):
        for j in range(g_ + l_):
            present, lane = lane_of(t, f, j, mode, size, crop_top)
            if not present:
                continue
            lane_pts[f, j] = len(lane)
            if len(lane) < 2:
                continue
            q = end_points(polyline(lane))
            lane_id = f * (g_ + l_) + j
            segs[lane_id, :len(q) - 1, :2] = q[:-1]
            segs[lane_id, :len(q) - 1, 2:4] = q[1:]
            segs[lane_id, :len(q) - 1, 4] = lane_id
    return segs, lane_pts


# ------------------------------------------------------------------------------------------------ count rules
def match(sim):
    """Kuhn-Munkres as the rules state it (the recursive search of the reference) -> (row_match, col_match, relabelling passes)."""
    n_r, n_c = len(sim), len(sim[0])
    swap = n_r > n_c
    mat = [[sim[j][i] for j in range(n_r)] for i in range(n_c)] if swap else sim
    ll, rr = len(mat), len(mat[0])
    lm, rm = [-1] * ll, [-1] * rr
    lw, rw = [], [0.0] * rr
    for i in range(ll):
        w = -1e5
        for j in range(rr):
            w = mat[i][j] if w < mat[i][j] else w
        lw.append(w)
    passes = 0

    def dfs(x, lu, ru):
        lu[x] = True
        for v in range(rr):
            if not ru[v] and abs(lw[x] + rw[v] - mat[x][v]) < 1e-2:
                ru[v] = True
                if rm[v] == -1 or dfs(rm[v], lu, ru):
                    rm[v] = x
                    lm[x] = v
                    return True
        return False

    for u in range(ll):
        stop = False
        while True:
            lu, ru = [False] * ll, [False] * rr
            if dfs(u, lu, ru):
                break
            dmin = 1e10
            for i in range(ll):
                for j in range(rr):
                    if lu[i] and not ru[j]:
                        d = lw[i] + rw[j] - mat[i][j]
                        dmin = d if d < dmin else dmin
            if dmin == 1e10:
                stop = True
                break
            passes += 1
            if passes > RELABEL_CAP:
                return None, None, passes
            for i in range(ll):
                if lu[i]:
                    lw[i] -= dmin
            for j in range(rr):
                if ru[j]:
                    rw[j] += dmin
        if stop:
            break
    return (rm, lm, passes) if swap else (lm, rm, passes)


def count_image(iou: np.ndarray, lane_pts: np.ndarray, threshold: float):
    """iou float64 [G,L], lane_pts int32 [G+L] -> dict(tp, fp, fn, iou_im, anno_match int32 [G], passes, overflow)."""
    g_, l_ = iou.shape
    rows = [g for g in range(g_) if lane_pts[g] >= 0]
    cols = [k for k in range(l_) if lane_pts[g_ + k] >= 0]
    am = np.full(g_, -1, np.int32)
    na, nd = len(rows), len(cols)
    res = dict(tp=0, fp=nd, fn=na, iou_im=0.0, anno_match=am, passes=0, overflow=0)
    if na == 0 and nd == 0:
        res["iou_im"] = 1.0
        return res
    if na == 0 or nd == 0:
        return res
    sim = [[0.0 if lane_pts[g] < 2 or lane_pts[g_ + k] < 2 else float(iou[g, k]) for k in cols] for g in rows]
    row_match, _, passes = match(sim)
    res["passes"] = passes
    if row_match is None:
        res["overflow"] = 1
        return res
    tp, total = 0, 0.0
    for r in range(na):
        c = row_match[r]
        if c >= 0:
            total += sim[r][c]
            if sim[r][c] > threshold:
                tp += 1
                am[rows[r]] = cols[c]
    res.update(tp=tp, fp=nd - tp, fn=na - tp, iou_im=total / nd)
    return res


def count_images(iou: np.ndarray, lane_pts: np.ndarray, threshold: float, video=None, totals=None, iou_tot=None):
    """The count kernel on F images: per-image arrays and the totals ADDED in ascending order -> dict."""
    f_, g_, _ = iou.shape
    n_rows = 1 if totals is None else len(totals)
    totals = np.zeros((n_rows, 4), np.int64) if totals is None else totals.copy()
    iou_tot = np.zeros(n_rows, f64) if iou_tot is None else iou_tot.copy()
    out = dict(tp=np.zeros(f_, np.int32), fp=np.zeros(f_, np.int32), fn=np.zeros(f_, np.int32), iou_im=np.zeros(f_, f64),
               anno_match=np.zeros((f_, g_), np.int32), passes=0, overflow=0)
    for f in range(f_):
        r = count_image(iou[f], lane_pts[f], threshold)
        for k in ("tp", "fp", "fn", "iou_im", "anno_match"):
            out[k][f] = r[k]
        out["passes"] = max(out["passes"], r["passes"])
        out["overflow"] += r["overflow"]
        v = 0 if video is None else int(video[f])
        if 0 <= v < len(totals):
            totals[v] += (r["tp"], r["fp"], r["fn"], 1)
            iou_tot[v] = iou_tot[v] + f64(r["iou_im"])
    out.update(totals=totals, iou_tot=iou_tot)
    return out


# ------------------------------------------------------------------------------------------------ cases
def _curve(x0, y0, x1, y1, n, bend=0.0, jitter=0.0, seed=0):
    """n points from (x0, y0) to (x1, y1) in evaluator coordinates, on a 1/8 grid (exact in float32 and in the wire inverse)."""
    r = np.random.default_rng(seed)
    s = np.linspace(0.0, 1.0, n)
    x = x0 + (x1 - x0) * s + bend * np.sin(np.pi * s) + (r.normal(0, jitter, n) if jitter else 0.0)
    y = y0 + (y1 - y0) * s
    return (np.rint(np.stack([x, y], 1) * 8) / 8).astype(f32)


def _to_wire(lane):
    """Evaluator coordinates -> the normalised float32 points the writer would have been given (last point first)."""
    lane = np.asarray(lane, f64)[::-1]
    return np.stack([lane[:, 0] / (SIZE[1] / 2), (lane[:, 1] * 2 - CROP_TOP) / SIZE[0]], 1).astype(f32)


def _tables(images, wire: bool, g=G, l=L, s=S, p=P):
    """images: [(annotations, predictions)] of evaluator-coordinate lanes -> the six input tables (numpy)."""
    f_ = len(images)
    t = dict(points=np.zeros((f_, l, s, 2), f32), count=np.zeros((f_, l), np.int32), lanes_num=np.zeros(f_, np.int32),
             gt_points=np.zeros((f_, g, p, 2), f32), gt_count=np.zeros((f_, g), np.int32), gt_num=np.zeros(f_, np.int32))
    for f, (anno, det) in enumerate(images):
        t["gt_num"][f], t["lanes_num"][f] = len(anno), len(det)
        for j, lane in enumerate(anno):
            lane = np.asarray(lane, f32).reshape(-1, 2)
            t["gt_count"][f, j] = len(lane)
            t["gt_points"][f, j, :len(lane)] = lane
        for k, lane in enumerate(det):
            lane = np.asarray(lane, f32).reshape(-1, 2)
            lane = _to_wire(lane) if wire and len(lane) else lane
            t["count"][f, k] = len(lane)
            t["points"][f, k, :len(lane)] = lane
    return t


def _images_regular():
    a0, a1, a2 = _curve(10, 46, 30, 10, P, bend=4), _curve(40, 46, 44, 12, 5, bend=-3), _curve(70, 44, 52, 14, 3)
    near = lambda lane, n, dx: _curve(lane[0, 0] + dx, lane[0, 1], lane[-1, 0] + dx, lane[-1, 1], n, bend=0.0)
    return [
        # more predictions than annotations: S points, 3 points, 2 points (dropped in wire mode), 4 points elsewhere
        ([a0, a1, a2], [_curve(10.5, 46, 30.5, 10, S, bend=4), near(a1, 3, 0.5), near(a2, 2, 0.25), _curve(5, 40, 75, 30, 4, bend=2)]),
        # more annotations than predictions (the transpose): annotations of 4, 2 and 1 points
        ([_curve(12, 44, 28, 12, 4, bend=2), _curve(50, 44, 60, 12, 2), _curve(30, 30, 30, 30, 1)],
         [_curve(50.5, 44, 60.5, 12, 5), _curve(12, 44, 28.5, 12, 6, bend=2)]),
        ([], [a0[:S], a1]),                                                  # no annotation
        ([a0, a2], []),                                                      # no prediction
        ([], []),                                                            # neither
        ([a0, _curve(20, 20, 20, 20, 0), a1], [_curve(10, 46, 30, 10, 5, bend=4), _curve(41, 46, 45, 12, 3, bend=-3)]),   # a 0-point lane
    ]


def _images_edge():
    rep = _curve(20, 44, 36, 12, 5)
    rep[2] = rep[1]                                                          # a repeated point: h = 0, NaN, end points 0
    bad = _curve(60, 44, 50, 12, 6)
    bad[1, 0], bad[3, 1], bad[4, 0] = np.inf, np.nan, -np.inf
    off_a, off_d = _curve(-500, -500, -400, -450, 4), _curve(900, 700, 950, 900, 3)
    one = _curve(30, 30, 30, 30, 1)
    twin = _curve(30, 46, 40, 10, 4, bend=2)
    ties = np.array([[1.25 * j, 9.25 + 1.25 * (31 - j)] for j in (3, 9, 17, 25, 31)], f32)     # x * 10, y * 10: exact halves
    return [
        ([rep, _curve(60, 44, 66, 12, 4)], [rep.copy(), _curve(60.5, 44, 66.5, 12, 4)]),
        ([bad, _curve(20, 44, 24, 12, 3)], [bad.copy(), _curve(20, 44, 24.5, 12, 4)]),
        ([off_a, one], [off_d, _curve(30, 40, 34, 12, 3)]),                  # empty masks: NaN IoU; the 1-point lane: 0, not NaN
        ([twin, twin.copy(), _curve(31, 46, 41, 10, 4, bend=2)], [twin.copy(), twin.copy(), _curve(30.5, 46, 40.5, 10, 5, bend=2)]),
        ([ties, _curve(60, 40, 62, 12, 3)], [ties.copy(), _curve(3.75, 46.75, 38.75, 10.5, 3)]),
    ]


def _over_limits(wire: bool):
    """Counts above (and below) the limits over tables that are full of points: clamped, never followed."""
    lanes = [_curve(8 + 9 * i, 46, 14 + 9 * i, 10, P, bend=1 + i) for i in range(G + L)]
    t = _tables([(lanes[:G], [lane[:S] for lane in lanes[G:]])], wire)
    t["gt_num"][0], t["lanes_num"][0] = 7, 9
    t["gt_count"][0], t["count"][0] = (100, -3, P), (50, S, -1, 3)
    big = _tables([(lanes[:G], [lane[:S] for lane in lanes[G:]])], wire)
    big["gt_num"][0], big["lanes_num"][0] = 2 ** 31 - 1, -2 ** 31
    big["gt_count"][0], big["count"][0] = (2 ** 31 - 1, -2 ** 31, 4), (2 ** 31 - 1, 5, 5, 5)
    return {k: np.concatenate([t[k], big[k]]) for k in t}


def table_cases():
    """[(name, mode, tables)]: F <= 6 images each."""
    raw_imgs = _images_regular()[:2] + _images_edge()[2:4]
    return [("regular", "wire", _tables(_images_regular(), True)), ("edge", "wire", _tables(_images_edge(), True)),
            ("limits", "wire", _over_limits(True)), ("raw", "raw", _tables(raw_imgs, False)),
            ("raw-edge", "raw", _tables(_images_edge(), False)), ("raw-limits", "raw", _over_limits(False))]


def full_geometry_case():
    """One case at the real geometry: 1280 x 1920, F = 2, S = 36, size (800, 1920), crop_top 480 -> (tables, options)."""
    r = np.random.default_rng(11)
    g, l, s, p = 4, 4, 36, 20
    imgs = []
    for f in range(2):
        anno = []
        for i in range(3 + f):
            n = (p, 12, 7, 3)[i]
            ys = np.linspace(1270, 520, n)
            anno.append((np.rint(np.stack([300 + 380 * i + np.cumsum(r.normal(0, 14, n)), ys], 1) * 2) / 2).astype(f32))
        det = []
        for i in range(4 - f):
            src = anno[i % len(anno)]
            ys = np.linspace(src[0, 1], src[-1, 1], (s, 20, 9, 3)[i])
            det.append(np.stack([np.interp(-ys, -src[:, 1], src[:, 0]) + 2.0 * i, ys], 1))
        imgs.append((anno, det))
    t = dict(points=np.zeros((2, l, s, 2), f32), count=np.zeros((2, l), np.int32), lanes_num=np.zeros(2, np.int32),
             gt_points=np.zeros((2, g, p, 2), f32), gt_count=np.zeros((2, g), np.int32), gt_num=np.zeros(2, np.int32))
    for f, (anno, det) in enumerate(imgs):
        t["gt_num"][f], t["lanes_num"][f] = len(anno), len(det)
        for j, lane in enumerate(anno):
            t["gt_count"][f, j] = len(lane)
            t["gt_points"][f, j, :len(lane)] = lane
        for k, lane in enumerate(det):
            lane = lane[::-1]
            t["count"][f, k] = len(lane)
            t["points"][f, k, :len(lane)] = np.stack([lane[:, 0] / 960.0, (lane[:, 1] * 2 - 480) / 800.0], 1).astype(f32)
    return t, dict(height=1280, width=1920, lane_width=30, threshold=0.5, size=(800, 1920), crop_top=480)


def matrix_cases():
    """[(name, iou float64 [F,G,L], lane_pts int32 [F,G+L])]: matrices for the count rules alone - ties and near-ties inside the
    1e-2 slack, NaN entries, empty sides, short lanes, the transpose, and 16 x 16."""
    nan = float("nan")
    out = []
    m = np.array([
        [[0.80, 0.805, 0.10, 0.0], [0.805, 0.80, 0.10, 0.0], [0.10, 0.10, 0.795, 0.79]],        # near-ties: the slack decides
        [[0.60, 0.60, 0.60, 0.60], [0.60, 0.60, 0.60, 0.60], [0.60, 0.60, 0.60, 0.60]],          # identical lanes
        [[nan, 0.70, 0.20, 0.0], [nan, nan, nan, nan], [0.30, 0.705, nan, 0.51]],                 # NaN: a row without a finite entry
        [[0.50, 0.5000001, 0.49, 0.0], [0.509, 0.50, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]],            # around the threshold
        [[0.90, 0.10, 0.10, 0.2], [0.89, 0.895, 0.10, 0.2], [0.895, 0.89, 0.885, 0.2]],           # a chain of re-matching
        [[0.30, 0.90, 0.20, 0.1], [0.10, 0.95, 0.40, 0.1], [0.20, 0.85, 0.10, 0.1]],              # one column wanted by all
    ], f64)
    pts = np.full((6, G + L), 5, np.int32)
    out.append(("slack", m, pts))
    pts2 = pts.copy()
    pts2[0, :] = (5, -1, 5, 5, 5, -1, -1)                   # 2 x 2 of a 3 x 4
    pts2[1, :] = (5, 5, 5, 5, -1, -1, -1)                   # 3 annotations, 1 prediction: the transpose
    pts2[2, :] = (-1, -1, -1, 5, 5, 1, 0)                   # no annotation
    pts2[3, :] = (5, 1, 0, -1, -1, -1, -1)                  # no prediction
    pts2[4, :] = -1                                         # neither
    pts2[5, :] = (1, 5, 5, 5, 0, 5, 1)                      # short lanes: sim 0 whatever iou holds
    out.append(("presence", m.copy(), pts2))
    r = np.random.default_rng(3)
    big = np.round(r.uniform(0, 1, (6, 16, 16)), 2)                                               # a 0.01 grid: many ties and near-ties
    big[1] = np.round(big[1] * 0.02 + 0.6, 3)
    big[2][r.uniform(size=(16, 16)) < 0.3] = nan
    big_pts = np.full((6, 32), 4, np.int32)
    big_pts[3, 5:16] = -1                                   # 5 x 16
    big_pts[4, 16 + 3:] = -1                                # 16 x 3: the transpose
    big_pts[5, ::3] = 1
    out.append(("16x16", big, big_pts))
    return out
