"""The three training criteria (csrc/loss.hip, csrc/loss_variants.hip, csrc/assign_device.h) as plain torch statements, for holding
the kernels to fp64 at every shape class they branch on.  CPU only: nothing here touches the GPU; tests/test_criterion_cpu.py
proves the cases and this harness on the CPU, tests/test_criterion_gpu.py uses them against the device.

A case is a `head_cases.Piece` per criterion (`piece(case, kind)`, kind = "v3" | "v1" | "v2"): seeded inputs (fp64 holding
fp32-representable values) and a statement that is generic in dtype - run in fp64 it is the reference, run in fp32 it is the
floor e32.  The statement returns the loss, the assignment cost of the six predictions (v3: its valid columns) and the
gradients of the loss with respect to the six prediction and three gate tensors (torch autograd, unit upstream) as OUTPUTS, so
`head_cases.compare` judges every one of them by its rule

    e_hip <= MARGIN * max(e32, median e32 over the case's tensors)       for ||.|| and max|.|

The integer results of the run (matched rows, pairs, k_j) are kept beside it (`integers`).

What the statements are made of: the cost matrices are oracle.phnet_cpu.assignment_cost / oracle.criterion_variants_cpu.
one2many_cost, the matching is scipy's on them, the terms are oracle.phnet_cpu.focal_vector / lane_iou_loss, F.smooth_l1_loss and
criterion_variants_cpu.line_iou_aligned.  The few lines that put them together are spelled out here instead of calling
O.frame_loss / OC.frame_loss_v1 / OC.frame_loss_v2, for three reasons: all SIX matchings are wanted (the oracle returns branch
B's), N < 4 must work (the oracle's topk(4) does not), and the matching must follow the kernels' documented tie rule where anchors
are identical (`canonical`).  tests/test_criterion_cpu.py shows them equal to the oracle's own functions at fp32 on `work`.

Contract of the kernels that the statements follow (include/phnet_hip.h): with fewer anchors than valid label rows nothing is
matched; labels are reported by their ORIGINAL row (the oracle filters the valid rows first and reports compact indices - the
mapping is done here, `Matching`)."""
import functools
from collections import OrderedDict
from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import criterion_variants_cpu as OC
from oracle import phnet_cpu as O
from tests.head_cases import STATEMENTS, Piece

LIOU = (7.5 / 768, 400.0, 960.0)                  # LaneIoU half width, image height / width: the class defaults of the reference
# Class logits of the saturated anchors: softmax at both ends and at equal large logits.  Logit 1 itself never sits at +20: the
# assignment cost takes log(1 - sigmoid(z1) + 1e-12), which in fp32 is log(1e-12) from z1 = 17 on and 0.7 off fp64 (2.5 % of
# the entry) - the fp32 floor of the whole cost tensor would be that one entry and the rule would hold the kernel to nothing.
SAT = ((-20.0, 0.3), (20.0, -20.0), (-20.0, -20.0), (20.0, 0.5))
NEAR_PER_LABEL = 6
TIE_COLS = (3, 17, 30)
GAP = 1e-3
K_MARGIN = 1e-2

# name, N, L, S, valid; near: six anchors on every valid label; off / dup as in tests/golden/make_goldens_assign_bits.py;
# scale: noise factor per label row of `near`; img: (w, h); kinds: the criteria the case is for
_C = lambda name, N, L, S, valid, **kw: dict(name=name, N=N, L=L, S=S, valid=[int(c) for c in valid], **kw)   # noqa: E731
CASES = [
    _C("work", 240, 4, 36, "1111", near=True, scale={1: 0.4, 2: 3.0}),
    _C("none", 240, 4, 36, "0000"),
    _C("whole", 240, 4, 36, "1111", off="whole"),
    _C("one", 1, 1, 3, "1"),
    _C("few", 3, 4, 4, "1010"),
    _C("short", 2, 4, 36, "1110"),
    _C("w63", 63, 2, 16, "11", near=True),
    _C("pf36", 64, 3, 38, "101"),
    _C("part", 65, 3, 18, "111", off="part"),
    _C("odd", 65, 3, 37, "111", near=True),
    _C("lane65", 65, 1, 65, "1"),
    _C("trip", 64, 4, 74, "1101", near=True),
    _C("s72", 256, 4, 72, "1111", near=True),
    _C("long", 256, 2, 250, "01"),
    _C("pair", 64, 4, 36, "1111", dup="pair"),
    _C("all", 65, 4, 16, "1011", dup="all"),
    _C("tie", 64, 2, 36, "11", near=True, img=(801, 321), kinds=("v1", "v2"), tie=True),
]
# seeds were chosen on the CPU so that the input conditions of tests/test_criterion_cpu.py hold (the fp64 reference alone decides)
RESEED = {"work": 1, "whole": 6, "odd": 1, "tie": 8}
for _i, _c in enumerate(CASES):
    for _k, _v in dict(near=False, off=None, dup=None, scale={}, img=(800, 320), kinds=("v3", "v1", "v2"), tie=False).items():
        _c.setdefault(_k, _v)
    _c["seed"] = 9100 + _i + 100 * RESEED.get(_c["name"], 0)
BY_NAME = {c["name"]: c for c in CASES}
KINDS = ("v3", "v1", "v2")
PAIRS = [(c["name"], k) for c in CASES for k in c["kinds"]]


def cost_path(S: int) -> str:
    """The cost path of lane_assign_block at S columns (assign_device.h: the dispatch after cost_phase)."""
    if S % 2:
        return "scalar"
    return "pf18" if S <= 36 else "pf36" if S <= 72 else "trips"


def n_valid(c) -> int:
    return sum(c["valid"])


def short(c) -> bool:
    """Fewer anchors than valid label rows: the kernels' precondition is violated and nothing is matched."""
    return c["N"] < n_valid(c)


# ------------------------------------------------------------------------------------------------ inputs
def _clear_edges(row: np.ndarray, trow: np.ndarray, img_w: int, keep=()):
    """Moves the x columns of an anchor that sits on a label (fp32 row, in place) by 0.05 px steps until no in-range column
    has |x - t| < 2e-2 px (the variants' fixed-radius IoU) or a LaneIoU interval end within 2e-5 of the label's (normalised): twice
    the margins of the input conditions, which tests/test_criterion_cpu.py checks on the finished inputs."""
    hw, ih, iw = LIOU
    S = row.shape[0] - 6
    t = trow[6:].astype(np.float64)
    ok = ~((t < 0) | (t >= img_w))
    dy = ih / (S - 1) * 2

    def widths(v):
        d = (v[2:] - v[:-2]) * iw
        d = np.where(np.abs(d) > 1e4, 0.0, d)
        wd = hw * np.sqrt(d * d + dy * dy) / dy
        return np.concatenate([wd[:1], wd, wd[-1:]])

    for _ in range(50):
        x = row[6:].astype(np.float64)
        bad = np.abs(x * (img_w - 1.0) - t) < 2e-2
        px, tt = x * (img_w - 1.0) / img_w, t / img_w
        pw, tw = widths(px), widths(tt)
        bad |= np.minimum(np.abs((px + pw) - (tt + tw)), np.abs((px - pw) - (tt - tw))) < 2e-5
        bad &= ok
        bad[list(keep)] = False
        if not bad.any():
            return
        row[6:][bad] += np.float32(0.05 / (img_w - 1.0))
    raise AssertionError("could not clear the IoU edges")


@functools.lru_cache(maxsize=None)
def _inputs(name: str) -> Dict[str, np.ndarray]:
    c = BY_NAME[name]
    r = np.random.default_rng(c["seed"])
    N, L, S = c["N"], c["L"], c["S"]
    img_w = c["img"][0]
    tgt = np.zeros((L, 6 + S), np.float32)
    tgt[:, 1] = np.asarray(c["valid"], np.float32)
    tgt[:, 2:5] = r.uniform(0.05, 0.95, (L, 3)).astype(np.float32)
    tgt[:, 5] = S
    xs = r.uniform(150, 650, (L, 1)) + r.normal(0, 6, (L, S)).cumsum(1)
    tgt[:, 6:] = np.clip(xs, 1.0, img_w - 2.0).astype(np.float32)
    if c["off"] in ("part", "whole"):
        tgt[0, 6:6 + (S + 2) // 3] = -2.0
        tgt[0, 6 + S - (S + 3) // 4:] = float(img_w)             # x == img_w is outside
    if c["off"] == "whole":
        tgt[2, 6:] = -1e5
    if c["tie"]:
        tgt[0, [6 + k for k in TIE_COLS]] = (img_w - 1) / 2.0

    base = r.normal(size=(N, 6 + S)) * 0.3 + 0.4
    base[:, :2] = r.normal(size=(N, 2))
    free = [i for i in r.permutation(N) if not (c["dup"] == "pair" and i in (5, 6))]
    sat, free = free[:len(SAT)], free[len(SAT):]
    near = {}                                                    # label row -> its anchors, the closest first
    if c["near"]:
        for j in range(L):
            if c["valid"][j]:
                near[j], free = free[:NEAR_PER_LABEL], free[NEAR_PER_LABEL:]
                for i, a in enumerate(near[j]):
                    sigma = 4.0 * (i + 1) * c["scale"].get(j, 1.0)
                    base[a, 6:] = tgt[j, 6:] / (img_w - 1.0) + r.normal(0, sigma, S) / (img_w - 1.0)
                    base[a, 2:5] = tgt[j, 2:5] + r.normal(0, 0.02, 3)
        sat[0] = near[min(near)][0]                              # the anchor with a saturated positive logit sits on a label
    if c["dup"] == "pair":                                       # the twins sit on label 1, so one of them is matched
        base[5, 6:] = tgt[1, 6:] / (img_w - 1.0) + r.normal(0, 4.0, S) / (img_w - 1.0)
        base[5, 2:5] = tgt[1, 2:5] + r.normal(0, 0.02, 3)
    placed = {j: list(v) for j, v in near.items()}               # anchors that sit on a label: their IoU edges are cleared below
    if c["dup"] == "pair":
        placed.setdefault(1, []).append(5)
    out = {"tgt": tgt}
    for q in range(6):
        p = base + r.normal(0, 0.002, base.shape)
        p[:, :2] = r.normal(size=(N, 2))                         # class logits: N(0, 1), drawn per tensor
        for i, a in enumerate(sat):                              # ... the first pattern stays on its anchor, the others rotate
            # over the stages of branch A only: the two branches of an anchor then differ, and its gate gradient is not 0
            p[a, :2] = SAT[0] if i == 0 else SAT[1 + (i - 1 + (q if q < 3 else 0)) % (len(SAT) - 1)]
        p = p.astype(np.float32)
        if c["tie"]:
            p[near[0][0], [6 + k for k in TIE_COLS]] = 0.5
        for j, anchors in placed.items():
            for a in anchors:
                _clear_edges(p[a], tgt[j], img_w, TIE_COLS if c["tie"] and a == near[0][0] and j == 0 else ())
        if c["dup"] == "pair":
            p[6] = p[5]
        if c["dup"] == "all":
            p[:] = p[0]
            p[:, :2] = SAT[1]
        out[f"pred{q}"] = p
    for q in range(3):
        out[f"gate{q}"] = r.uniform(0.3, 0.9, N).astype(np.float32)
    out["_near0"] = np.asarray([near[0][0]] if c["tie"] else [-1])
    return out


def inputs(name: str) -> Dict[str, torch.Tensor]:
    """{pred0..5 [N,6+S], gate0..2 [N], tgt [L,6+S]} as fp64 tensors holding fp32 values."""
    return {k: torch.from_numpy(v).double() for k, v in _inputs(name).items() if not k.startswith("_")}


def tie_anchor(name: str) -> int:
    return int(_inputs(name)["_near0"][0])


def geometry(c) -> O.Geometry:
    return O.Geometry(img_w=c["img"][0], img_h=c["img"][1], num_points=c["S"], num_priors=c["N"])


# ------------------------------------------------------------------------------------------------ matching
def solve(C: torch.Tensor) -> Tuple[List[int], List[int], float]:
    """scipy's optimum of a [n, m] matrix (n >= m): rows ascending, their columns, the total."""
    r, c = O.hungarian(C)
    return r.tolist(), c.tolist(), float(C[r, c].double().sum())


def runner_up(C: torch.Tensor, rows, cols) -> float:
    """Total of the best assignment that differs from (rows, cols): the optimum with one of its pairs forbidden, the best over
    the pairs (the first partition of Murty's ranking).  inf where no other complete assignment exists."""
    best = float("inf")
    big = 1e6
    for i, j in zip(rows, cols):
        D = C.clone()
        D[i, j] = big
        _, _, tot = solve(D)
        if tot < big / 2:
            best = min(best, tot)
    return best


def canonical(pred: torch.Tensor, rows: List[int], cols: List[int], free: List[bool], dup: bool = True) -> Tuple[List[int], List[int]]:
    """The kernels' tie rule among assignments of equal cost (assign_device.h: each column ranks its rows by (cost, index), the
    combination of lowest index sum(rank_j * 4^j) wins): identical anchors have identical costs, so the label of the HIGHEST row
    takes the lowest-indexed free anchor of a group of identical anchors first.  Returns the pairs sorted by anchor."""
    if not dup:
        pairs = sorted(zip(rows, cols))
        return [p[0] for p in pairs], [p[1] for p in pairs]
    taken = set()
    out = {}
    for j, i in sorted(zip(cols, rows), reverse=True):
        twins = [a for a in range(pred.shape[0]) if free[a] and a not in taken and torch.equal(pred[a], pred[i])]
        out[j] = twins[0]
        taken.add(twins[0])
    pairs = sorted((i, j) for j, i in out.items())
    return [p[0] for p in pairs], [p[1] for p in pairs]


class Matching:
    """One prediction tensor's assignments in the layout of the device, from cost matrices in the statement's dtype.
    one-to-one: cost [N, m] (valid columns), rows / cols (compact, by anchor), rows_by_col [L], rows_sorted [L], n_valid;
    one-to-many: many_rows / many_cols [16] (ORIGINAL label rows, round order, -1 padded), many_n, ks (per valid label),
    sums (their top-4 IoU sums), iou_max (largest raw IoU per valid label), and per solved matrix (C, rows, cols) in `solved`."""

    def __init__(self, c, pred: torch.Tensor, tgt: torch.Tensor):
        g = geometry(c)
        N, L = c["N"], c["L"]
        orig = [j for j in range(L) if c["valid"][j]]
        m = len(orig)
        tg = tgt[orig]
        self.solved = []
        self.cost = O.assignment_cost(pred, tg, g) if m else pred.new_zeros(N, 0)
        self.rows, self.cols = [], []
        self.many = []
        self.ks, self.sums, self.iou_max = [], [], []
        if m:
            C, iou = OC.one2many_cost(pred, tg, g)
            self.iou_max = iou.max(dim=0)[0].tolist()
            self.sums = torch.topk(iou.clamp(min=0.0), min(4, N), dim=0)[0].sum(0).tolist()
            self.ks = [max(1, int(s)) for s in self.sums]
        if m and not short(c):
            free = [True] * N
            r, cc, _ = solve(self.cost)
            self.solved.append((self.cost, r, cc))
            self.rows, self.cols = canonical(pred, r, cc, free, bool(c['dup']))
            ks = list(self.ks)
            C = C.clone()
            while sum(ks) > 0 and sum(free) >= m:
                r, cc, _ = solve(C)
                self.solved.append((C.clone(), r, cc))
                r, cc = canonical(pred, r, cc, free, bool(c['dup']))
                for p in range(m):                               # as shipped: the per-label mask indexes the row-sorted pair list
                    if ks[p] > 0:
                        self.many.append((r[p], orig[cc[p]]))
                        free[r[p]] = False
                        C[r[p], :] = OC.INFINITY
                ks = [k - 1 if k > 0 else k for k in ks]
        self.rows_by_col = [-1] * L
        for i, j in zip(self.rows, self.cols):
            self.rows_by_col[orig[j]] = i
        self.rows_sorted = sorted(self.rows) + [-1] * (L - len(self.rows))
        self.n_valid = len(self.rows)
        self.many_rows = [p[0] for p in self.many] + [-1] * (16 - len(self.many))
        self.many_cols = [p[1] for p in self.many] + [-1] * (16 - len(self.many))
        self.many_n = len(self.many)
        self.orig = orig


# ------------------------------------------------------------------------------------------------ statements
def _lane_iou(pred: torch.Tensor, tgt: torch.Tensor, bug: str) -> torch.Tensor:
    if bug != "width_k0":
        return O.lane_iou_loss(pred[:, 6:], tgt[:, 6:], *LIOU)
    # the perturbation "width from column k instead of the clamped neighbour at k = 0": the kernel's index c = k reads the
    # elements before and after column 0 of the ROW, i.e. column 5 (the length) and x column 1
    hw, ih, iw = LIOU
    p, t = pred[:, 6:], tgt[:, 6:]
    dy = ih / (p.shape[1] - 1) * 2
    pd = torch.cat([(pred[:, 7:8] - pred[:, 5:6]), p[:, 2:] - p[:, :-2], (p[:, -1:] - p[:, -3:-2])], dim=1).detach() * iw
    pw = hw * torch.sqrt(pd.pow(2) + dy ** 2) / dy
    td = (t[:, 2:] - t[:, :-2]) * iw
    td = torch.where(td.abs() > 1e4, torch.zeros_like(td), td)
    tw = hw * torch.sqrt(td.pow(2) + dy ** 2) / dy
    tw = torch.cat([tw[:, :1], tw, tw[:, -1:]], dim=1)
    ovr = (torch.min(p + pw, t + tw) - torch.max(p - pw, t - tw)).masked_fill((t < 0) | (t >= 1.0), 0.0)
    uni = (torch.max(p + pw, t + tw) - torch.min(p - pw, t - tw)).masked_fill((t < 0) | (t >= 1.0), 0.0)
    return (1 - ovr.sum(-1) / (uni.sum(-1) + 1e-9)).mean()


def _median(x: torch.Tensor, bug: str) -> torch.Tensor:
    if bug == "upper_median":
        return x.detach().sort()[0][x.numel() // 2]
    return torch.median(x).detach()                              # the lower median


def _criterion(kind: str, t: Dict[str, torch.Tensor], opts: dict):
    c, bug = BY_NAME[opts["case"]], opts.get("bug", "")
    g = geometry(c)
    N, L, S, w = c["N"], c["L"], c["S"], c["img"][0]
    preds = [t[f"pred{q}"].detach().clone().requires_grad_(True) for q in range(6)]
    gates = [t[f"gate{q}"].detach().clone().requires_grad_(True) for q in range(3)]
    tgt = t["tgt"]
    dtype = tgt.dtype
    M = [Matching(c, p.detach(), tgt) for p in preds]
    m = n_valid(c)
    tg = tgt[M[0].orig]
    scale = torch.tensor([S - 1.0, w - 1.0, 180.0, S - 1.0], dtype=dtype)
    wrong_m = (m / L) if bug == "m_is_L" else 1.0                # the perturbation "divisor m replaced by L"

    def smooth(pred, rows, cols):
        return F.smooth_l1_loss(pred[rows, 2:6] * scale, tg[cols, 2:6] * scale, reduction="none")

    def branch(qs):
        cls, reg, iou, last = 0.0, 0.0, 0.0, []
        for q in qs:
            pred = preds[q]
            rows, cols = (M[q].rows, M[q].cols) if kind != "v2" else ([p[0] for p in M[q].many], [M[q].orig.index(p[1]) for p in M[q].many])
            labels = torch.zeros(N, dtype=torch.long)
            labels[rows] = 1
            cls = cls + O.focal_vector(pred[:, :2], labels)
            last = rows
            if not rows:
                continue
            if kind == "v3":                                     # loss4OLV3.py:34-82
                reg = reg + smooth(pred, rows, cols).mean() * wrong_m
                iou = iou + _lane_iou(torch.cat([pred[rows, :6] * (w - 1) / w, pred[rows, 6:] * (w - 1) / w], 1), torch.cat([tg[cols, :6], tg[cols, 6:] / w], 1), bug) * wrong_m
            elif kind == "v1":                                   # loss4OL.py:88-166: per pair, by position in the row-sorted list
                reg = reg + smooth(pred, rows, cols).mean(-1) / len(rows) * wrong_m
                iou = iou + (1 - OC.line_iou_aligned(pred[rows, 6:] * (w - 1), tg[cols, 6:], w, 15.0)) / len(rows) * wrong_m
            else:                                                # loss4OLV2.py:28-93: means over all pairs
                reg = reg + smooth(pred, rows, cols).mean()
                iou = iou + (1 - OC.line_iou_aligned(pred[rows, 6:] * (w - 1), tg[cols, 6:], w, 15.0)).mean()
        return cls / 3, reg / 3, iou / 3, last

    with torch.enable_grad():
        cls_a, reg_a, iou_a, last_a = branch((0, 1, 2))
        cls_b, reg_b, iou_b, last_b = branch((3, 4, 5))
        d = torch.stack(gates, dim=0).mean(dim=0)
        if kind == "v1":                                         # loss4OL.py:168-232: the pair terms land on the last stage's anchors
            def inst(cls, reg, iou, last):
                v = cls * g.cls_weight
                if not last:
                    return v
                add = torch.zeros_like(v)
                add[last] = reg * g.reg_weight + iou * g.iou_weight
                return v + add
            la, lb = inst(cls_a, reg_a, iou_a, last_a), inst(cls_b, reg_b, iou_b, last_b)
            delta = _median(la - lb, bug)
            loss = torch.sum((1 - d) * (la - delta / 2) + d * (lb + delta / 2))
        else:
            delta = _median(cls_a - cls_b, bug)
            cls = torch.sum((1 - d) * (cls_a - delta / 2) + d * (cls_b + delta / 2))
            half = 0.5 if kind == "v2" else 1.0
            loss = (reg_a + reg_b) * g.reg_weight * half + (iou_a + iou_b) * g.iou_weight * half + cls * g.cls_weight
        grads = torch.autograd.grad(loss, preds + gates, allow_unused=True)
    grads = [torch.zeros_like(x) if gr is None else gr for x, gr in zip(preds + gates, grads)]
    outs = OrderedDict(loss=loss.detach().reshape(1))
    if kind == "v3" and m:
        for q in range(6):
            outs[f"cost{q}"] = M[q].cost
    for q in range(6):
        outs[f"dpred{q}"] = grads[q]
    for q in range(3):
        outs[f"dgate{q}"] = grads[6 + q]
    _INTS[(c["name"], kind, dtype, bug)] = M
    return outs


_INTS: Dict[tuple, List[Matching]] = {}
for _kind in KINDS:
    STATEMENTS["criterion_" + _kind] = functools.partial(lambda t, relu, o, kind: _criterion(kind, t, o), kind=_kind)


@functools.lru_cache(maxsize=None)
def piece(name: str, kind: str, bug: str = "") -> Piece:
    c = BY_NAME[name]
    return Piece(name=f"{name}-{kind}" + (f"-{bug}" if bug else ""), kind="criterion_" + kind, seed=c["seed"], tensors=inputs(name), params=(),
                 opts=dict(case=name, bug=bug))


def matchings(name: str, kind: str, dtype=torch.float64) -> List[Matching]:
    """The six Matching objects of the statement's run in `dtype` (the run is made and cached by head_cases)."""
    from tests.head_cases import reference_and_floor
    reference_and_floor(piece(name, kind))
    return _INTS[(name, kind, dtype, "")]


def integers(name: str, kind: str, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """What the loss entry points report besides floats, in their layout: v3: rows_by_col / rows_sorted [6, L]; v1: pair_rows /
    pair_cols [6, 16] (entry j = label row j) and rows_sorted [6, L]; v2: pair_rows / pair_cols [6, 16] (round order)."""
    M = matchings(name, kind, dtype)
    i64 = lambda rows: torch.tensor(rows, dtype=torch.int64)     # noqa: E731
    if kind == "v3":
        return dict(rows_by_col=i64([x.rows_by_col for x in M]), rows_sorted=i64([x.rows_sorted for x in M]))
    if kind == "v1":
        L = BY_NAME[name]["L"]
        return dict(pair_rows=i64([x.rows_by_col + [-1] * (16 - L) for x in M]),
                    pair_cols=i64([[j if x.rows_by_col[j] >= 0 else -1 for j in range(L)] + [-1] * (16 - L) for x in M]),
                    rows_sorted=i64([x.rows_sorted for x in M]))
    return dict(pair_rows=i64([x.many_rows for x in M]), pair_cols=i64([x.many_cols for x in M]))


def exact_zeros(name: str, kind: str, outs: Dict[str, torch.Tensor]) -> List[tuple]:
    """Entries of dpred that the fp64 statement makes exactly zero (columns 2.. of unmatched anchors, the out-of-image columns
    of matched ones) and `outs` does not: [(tensor, count)]."""
    from tests.head_cases import reference_and_floor
    ref, _ = reference_and_floor(piece(name, kind))
    bad = []
    for q in range(6):
        k = f"dpred{q}"
        n = int(((ref.outs[k] == 0) & (outs[k] != 0)).sum())
        if n:
            bad.append((k, n))
    return bad
