"""tests/criterion_cases.py proved on the CPU: the input conditions under which an fp32 kernel and the fp64 statement must take the
same discrete decisions hold for every case (checked on the fp64 reference ALONE - they are conditions on the inputs, not
tolerances), the case list covers what the kernels branch on, the spelled-out statements equal the oracle's own functions, the
fp32 run of the statement passes `compare` against the fp64 run, and `compare` rejects kernels that are subtly wrong.

Rejected perturbations of the fp32 run (error / bound of the named tensor, relative L2; measured here on the CPU):

    divisor m replaced by L (trip: m = 3, L = 4)    v3 loss 2.5e-01 / 7.2e-07    v1 loss 2.4e-01 / 3.3e-07    (dpred0 alike)
    upper instead of lower median (pair: N = 64)    v3 dgate 9.0e-03 / 1.1e-06   v1 dgate 3.9e-04 / 4.3e-07   v2 dgate 2.3e-02 / 1.1e-06
    LaneIoU width at k = 0 from column k (work)     v3 dpred0 3.2e-02 / 8.4e-07
    dgate * (1 + 1e-4) (work)                       v3 1.0e-04 / 8.4e-07   v1 1.0e-04 / 5.5e-07   v2 1.0e-04 / 6.8e-07
    a pair's gradient row on the twin anchor (pair) v3 1.4e+00 / 4.9e-07   v1 1.5e+00 / 2.6e-07   v2 1.4e+00 / 2.3e-07
"""
import pytest
import torch

from oracle import criterion_variants_cpu as OC
from oracle import phnet_cpu as O
from tests import criterion_cases as CC
from tests.head_cases import compare, reference_and_floor

NAMES = [c["name"] for c in CC.CASES]


def _in_range(t, w):
    return ~((t < 0) | (t >= w))


# ------------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("name", NAMES)
def test_label_xs_have_one_in_range_answer(name):
    c = CC.BY_NAME[name]
    w = c["img"][0]
    xs = CC.inputs(name)["tgt"][:, 6:]
    assert bool((((xs >= 1) & (xs <= w - 2)) | (xs == w) | (xs < 0)).all())


@pytest.mark.parametrize("name", NAMES)
def test_matching_gap_and_kj_margin(name):
    c = CC.BY_NAME[name]
    M = CC.matchings(name, c["kinds"][0])
    t = CC.inputs(name)
    for q, x in enumerate(M):
        pred = t[f"pred{q}"]
        for C, r, cc in x.solved:
            tot = float(C[r, cc].sum())
            if not c["dup"]:
                gap = CC.runner_up(C, r, cc) - tot
                assert gap >= CC.GAP, (name, q, gap)
        if c["dup"] and x.solved:
            # duplicate anchors tie exactly in every precision: the matching's total is the optimum, and no matched anchor has
            # an identical unmatched twin of lower index
            C, r, cc = x.solved[0]
            assert abs(float(C[x.rows, x.cols].sum()) - float(C[r, cc].sum())) <= 1e-12
            for matched in (set(x.rows), {p[0] for p in x.many}):
                for a in matched:
                    assert not any(b not in matched and torch.equal(pred[a], pred[b]) for b in range(a)), (name, q, a)
        for s, top in zip(x.sums, x.iou_max):
            # a top-4 sum of exactly 0 is exempt where it is 0 in every precision: every raw IoU of the label is clearly negative
            # (clamped to 0), or the label has no column inside the image (0 / 1e-9)
            assert abs(s - round(s)) >= CC.K_MARGIN or (s == 0.0 and (top <= -CC.K_MARGIN or top == 0.0)), (name, q, s, top)


@pytest.mark.parametrize("name,kind", CC.PAIRS)
def test_iou_edges_of_matched_pairs(name, kind):
    """No min / max of a matched pair's IoU terms sits where rounding could choose the other branch (except `tie`, where it sits
    there exactly in every precision)."""
    c = CC.BY_NAME[name]
    w = c["img"][0]
    t = CC.inputs(name)
    tgt = t["tgt"]
    seen_tie = 0
    for q, x in enumerate(CC.matchings(name, kind)):
        pred = t[f"pred{q}"]
        pairs = x.many if kind == "v2" else [(i, x.orig[j]) for i, j in zip(x.rows, x.cols)]
        for a, j in pairs:
            if kind == "v3":
                hw, ih, iw = CC.LIOU
                p, tt = pred[a, 6:] * (w - 1) / w, tgt[j, 6:] / w
                dy = ih / (c["S"] - 1) * 2
                width = lambda v: (lambda d: hw * torch.sqrt(torch.where(d.abs() > 1e4, torch.zeros_like(d), d).pow(2) + dy ** 2) / dy)(  # noqa: E731
                    (v[2:] - v[:-2]) * iw)
                pw, tw = width(p), width(tt)
                pw, tw = torch.cat([pw[:1], pw, pw[-1:]]), torch.cat([tw[:1], tw, tw[-1:]])
                ok = _in_range(tt, 1.0)
                edge = torch.minimum(((p + pw) - (tt + tw)).abs(), ((p - pw) - (tt - tw)).abs())[ok]
                assert edge.numel() == 0 or float(edge.min()) >= 1e-5, (name, q, a, j, float(edge.min()))
            else:
                dist = (pred[a, 6:] * (w - 1) - tgt[j, 6:]).abs()
                ok = _in_range(tgt[j, 6:], w)
                if c["tie"] and a == CC.tie_anchor(name) and j == 0:
                    assert bool((dist[list(CC.TIE_COLS)] == 0).all())
                    assert bool((pred[a, 6:].float().double() * (w - 1) == tgt[j, 6:])[list(CC.TIE_COLS)].all())
                    ok[list(CC.TIE_COLS)] = False
                    seen_tie += 1
                assert not bool(ok.any()) or float(dist[ok].min()) >= 1e-2, (name, q, a, j, float(dist[ok].min()))
    if c["tie"]:
        assert seen_tie == 6, "the anchor with x == t is matched to label 0 by every one of the six predictions"


# ------------------------------------------------------------------------------------------------ coverage
def test_the_cases_cover_what_the_kernels_branch_on():
    assert {CC.cost_path(c["S"]) for c in CC.CASES} == {"pf18", "pf36", "trips", "scalar"}
    assert {c["S"] for c in CC.CASES if CC.cost_path(c["S"]) == "pf36"} >= {38, 72}
    assert {c["N"] for c in CC.CASES} >= {1, 2, 3, 63, 64, 65, 240, 256}
    assert {c["L"] for c in CC.CASES} == {1, 2, 3, 4}
    assert any(c["S"] > 64 and c["S"] % 2 for c in CC.CASES) and any(c["S"] == 3 for c in CC.CASES)
    ks = set()
    for c in CC.CASES:
        for x in CC.matchings(c["name"], c["kinds"][0]):
            ks |= set(x.ks)
    assert ks >= {1, 2, 3}
    work = CC.matchings("work", "v2")
    assert all({1, 3} <= set(x.ks) for x in work)
    assert all(4 <= x.many_n <= 8 for n in ("work", "w63", "odd", "trip", "s72") for x in CC.matchings(n, "v2"))
    trip = CC.matchings("trip", "v2")[0]
    assert 3 in trip.many_cols and 2 not in trip.many_cols       # original label row 3 is compact index 2
    assert CC.short(CC.BY_NAME["short"]) and not any(CC.short(c) for c in CC.CASES if c["name"] != "short")
    assert all(x.n_valid == 0 and x.many_n == 0 for x in CC.matchings("short", "v3"))


# ------------------------------------------------------------------------------------------------ the statements
def _oracle_args(t):
    fir = [t[f"pred{q}"].unsqueeze(0) for q in range(3)]
    sec = [t[f"pred{q}"].unsqueeze(0) for q in range(3, 6)]
    gates = [t[f"gate{q}"].view(1, -1, 1) for q in range(3)]
    return fir, sec, gates, t["tgt"].unsqueeze(0)


@pytest.mark.parametrize("kind", CC.KINDS)
def test_statement_equals_the_oracle_at_fp32_on_work(kind):
    """The spelled-out statement against O.frame_loss / OC.frame_loss_v1 / OC.frame_loss_v2 themselves: the loss, every gradient
    and branch B's matched anchors, at fp32, to the last bit."""
    c = CC.BY_NAME["work"]
    g = CC.geometry(c)
    t = {k: v.float().requires_grad_(k != "tgt") for k, v in CC.inputs("work").items()}
    fir, sec, gates, gt = _oracle_args(t)
    if kind == "v3":
        mb, loss = O.frame_loss(O.FrameOutput(fir, sec, [], gates), gt, g)
    elif kind == "v1":
        mb, loss = OC.frame_loss_v1(fir, sec, gates, gt, g)
    else:
        mb, loss, _ = OC.frame_loss_v2(fir, sec, gates, gt, g)
    names = [f"pred{q}" for q in range(6)] + [f"gate{q}" for q in range(3)]
    grads = torch.autograd.grad(loss, [t[k] for k in names])
    _, floor = reference_and_floor(CC.piece("work", kind))
    assert torch.equal(floor.outs["loss"], loss.detach().reshape(1))
    for k, gr in zip(names, grads):
        assert torch.equal(floor.outs["d" + k], gr), k
    M = CC.matchings("work", kind, torch.float32)
    for q in range(3):
        mine = [p[0] for p in M[3 + q].many] if kind == "v2" else M[3 + q].rows
        assert mine == mb[q].tolist()
    if kind == "v3":                                              # ... and the cost is the oracle's function called as it is
        for q in range(6):
            assert torch.equal(floor.outs[f"cost{q}"], O.assignment_cost(t[f"pred{q}"].detach(), t["tgt"], g))
    if kind == "v2":                                              # the one-to-many rounds against the oracle's loop, compact -> original
        for q in range(6):
            r, cc = OC.assign_one2many(t[f"pred{q}"].detach(), t["tgt"], g)
            assert r.tolist() == [p[0] for p in M[q].many] and [M[q].orig[j] for j in cc.tolist()] == [p[1] for p in M[q].many]


@pytest.mark.parametrize("name", ["odd", "trip"])
def test_one2many_rounds_equal_the_oracle_off_the_workload_shape(name):
    c = CC.BY_NAME[name]
    t = CC.inputs(name)
    valid = [j for j in range(c["L"]) if c["valid"][j]]
    for q, x in enumerate(CC.matchings(name, "v2")):
        r, cc = OC.assign_one2many(t[f"pred{q}"], t["tgt"][valid], CC.geometry(c))
        assert r.tolist() == [p[0] for p in x.many] and [valid[j] for j in cc.tolist()] == [p[1] for p in x.many]


@pytest.mark.parametrize("name,kind", CC.PAIRS)
def test_fp32_run_passes_compare(name, kind):
    p = CC.piece(name, kind)
    _, floor = reference_and_floor(p)
    rep = compare(p, floor.outs, {})
    assert not rep.bad, rep.bad
    assert not CC.exact_zeros(name, kind, floor.outs)
    for k, v in CC.integers(name, kind).items():
        assert torch.equal(v, CC.integers(name, kind, torch.float32)[k]), k


# ------------------------------------------------------------------------------------------------ compare rejects wrong kernels
def _fp32_run(name, kind, bug=""):
    t = {k: v.float() for k, v in CC.inputs(name).items()}
    return {k: v.clone() for k, v in CC._criterion(kind, t, dict(case=name, bug=bug)).items()}


def _rejected(name, kind, outs, where):
    rep = compare(CC.piece(name, kind), outs, {})
    hit = [b for b in rep.bad if b[0].startswith("out:" + where)]
    assert hit, (name, kind, where, rep.bad)
    print(f"{name} {kind}: rejected at {[(b[0], b[1], f'{b[2]:.1e} / {b[3]:.1e}') for b in hit[:2]]}")


@pytest.mark.parametrize("kind", ["v3", "v1"])
def test_compare_rejects_divisor_L_for_m(kind):
    assert CC.n_valid(CC.BY_NAME["trip"]) == 3 and CC.BY_NAME["trip"]["L"] == 4
    outs = _fp32_run("trip", kind, "m_is_L")
    _rejected("trip", kind, outs, "loss")
    _rejected("trip", kind, outs, "dpred")


@pytest.mark.parametrize("kind", CC.KINDS)
def test_compare_rejects_the_upper_median(kind):
    assert CC.BY_NAME["pair"]["N"] % 2 == 0
    _rejected("pair", kind, _fp32_run("pair", kind, "upper_median"), "dgate")


def test_compare_rejects_a_laneiou_width_from_column_k_at_k0():
    _rejected("work", "v3", _fp32_run("work", "v3", "width_k0"), "dpred")


@pytest.mark.parametrize("kind", CC.KINDS)
def test_compare_rejects_dgate_off_by_1e4(kind):
    outs = _fp32_run("work", kind)
    outs["dgate1"] = outs["dgate1"] * (1 + 1e-4)
    _rejected("work", kind, outs, "dgate1")


@pytest.mark.parametrize("kind", CC.KINDS)
def test_compare_rejects_a_gradient_row_on_the_twin_anchor(kind):
    M = CC.matchings("pair", kind)
    q = 4
    matched = {p[0] for p in M[q].many} if kind == "v2" else set(M[q].rows)
    assert matched & {5, 6}
    outs = _fp32_run("pair", kind)
    g = outs[f"dpred{q}"]
    g[[5, 6], 2:] = g[[6, 5], 2:]
    _rejected("pair", kind, outs, f"dpred{q}")
    assert CC.exact_zeros("pair", kind, outs) or matched >= {5, 6}
