"""The criterion kernels (csrc/loss.hip, csrc/loss_variants.hip, csrc/assign_device.h) against the fp64 statements of
tests/criterion_cases.py, at every shape class they branch on.  Run with -m gpu.

Per case and criterion: the loss, the six cost matrices (v3), the six prediction gradients and the three gate gradients are held
to  e_hip <= 4 * max(e32, median e32 over the case's tensors)  for ||.|| and max|.| (head_cases.compare; e32 = the same
statement in torch fp32 on the CPU); entries the statement makes exactly zero are zero; matched rows, pairs, their order and
padding are equal.  `short` (fewer anchors than valid label rows) pins the contract of include/phnet_hip.h: no match at all.

UNMEASURED: this file has not run on an MI355X yet, so the table of device error against e32 (median / max over the case's
tensors, per case and criterion) is still missing here; every test prints its line of that table, with the case's cost path and
k_j (pytest -s).  Known from the CPU alone - the cost path of lane_assign_block per case (lane_assign_tokens caps the register
row at 36 columns, so it takes the trips path at S = 38 and 72):

    pf18: work none whole few short w63 part pair all tie     pf36: pf36 s72     trips: trip long     scalar: one odd lane65

k_j: {1, 2, 3} in work, 2 in the other near cases, 1 elsewhere (tests/test_criterion_cpu.py asserts the coverage); the fp32
floors e32 are 1e-7 to 2e-5 per tensor on the CPU.
"""
import ctypes

import pytest
import torch

from tests import criterion_cases as CC
from tests.head_cases import compare

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in CC.CASES]
PAD = 64                       # elements behind every output
I64_SENT, F32_SENT = -7777, 0x7FC12345        # the float sentinel is a NaN with a payload of its own
ERR_ARG = -1


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from phnet_amd import hip_ops
    return hip_ops


def _dev(name):
    t = {k: v.float().cuda() for k, v in CC.inputs(name).items()}
    return [t[f"pred{q}"] for q in range(6)], [t[f"gate{q}"] for q in range(3)], t["tgt"]


def _weights(c):
    g = CC.geometry(c)
    return g.cls_weight, g.reg_weight, g.iou_weight


def _cpu(x):
    return x.detach().cpu()


def _judge(name, kind, outs):
    rep = compare(CC.piece(name, kind), outs, {})
    c = CC.BY_NAME[name]
    ks = sorted({k for x in CC.matchings(name, kind) for k in x.ks})
    print(f"\n    {name:7s} {kind}  {rep.line(CC.cost_path(c['S']) + f' k_j {ks}')}")
    assert not rep.bad, rep.bad
    assert not CC.exact_zeros(name, kind, outs)


# ------------------------------------------------------------------------------------------------ assignment
@pytest.mark.parametrize("name", NAMES)
def test_assignment_integers_and_invalid_columns(K, name):
    """lane_assign, lane_assign_tokens and lane_assign_one2many on each of the six predictions: every integer output equals the
    fp64 statement's; cost columns of invalid label rows are +inf (the valid ones are judged with the v3 criterion below)."""
    c = CC.BY_NAME[name]
    w, h = c["img"]
    preds, _, tgt = _dev(name)
    L, E = c["L"], 16
    feat = torch.randn(c["N"], E, device="cuda")
    M = CC.matchings(name, c["kinds"][0])
    for q, x in enumerate(M):
        rows, srt, nv, cost = K.lane_assign(preds[q], tgt, w, h, want_cost=True)
        assert _cpu(rows).tolist() == x.rows_by_col and _cpu(srt).tolist() == x.rows_sorted and int(nv) == x.n_valid, (q, _cpu(rows), x.rows_by_col)
        cost = _cpu(cost)
        for j in range(L):
            if not c["valid"][j]:
                assert bool((cost[:, j] == float("inf")).all()), (q, j)
        assert bool(torch.isfinite(cost[:, x.orig]).all())
        tokens, valid = torch.zeros(L + 1, E, device="cuda"), torch.zeros(L + 1, dtype=torch.bool, device="cuda")
        assert _cpu(K.lane_assign_tokens(preds[q], tgt, w, h, feat, (tokens, valid))).tolist() == x.rows_sorted
        assert _cpu(valid).tolist() == [r >= 0 for r in x.rows_sorted] + [True]
        mr, mc, mn = K.lane_assign_one2many(preds[q], tgt, w, h)
        assert _cpu(mr).tolist() == x.many_rows and _cpu(mc).tolist() == x.many_cols and int(mn) == x.many_n, (q, _cpu(mr), x.many_rows, _cpu(mc), x.many_cols)


def test_short_reports_no_match_at_all(K):
    """Fewer anchors (2) than valid label rows (3): rows -1, n_valid 0, no pairs from all four entry points; the losses are the
    classification terms alone (the statement of `short`, judged below, has no other term)."""
    c = CC.BY_NAME["short"]
    w, h = c["img"]
    preds, gates, tgt = _dev("short")
    L = c["L"]
    for p in preds:
        rows, srt, nv, cost = K.lane_assign(p, tgt, w, h, want_cost=True)
        assert _cpu(rows).tolist() == [-1] * L and _cpu(srt).tolist() == [-1] * L and int(nv) == 0
        mr, mc, mn = K.lane_assign_one2many(p, tgt, w, h)
        assert _cpu(mr).tolist() == [-1] * 16 and _cpu(mc).tolist() == [-1] * 16 and int(mn) == 0
    _, dpred, _, rows, srt = K.frame_loss(preds, gates, tgt, w, h, *_weights(c), *CC.LIOU)
    assert bool((rows == -1).all()) and bool((srt == -1).all()) and bool((dpred[:, :, 2:] == 0).all())
    for variant in (1, 2):
        _, dpred, _, prow, pcol, _ = K.frame_loss_variant(variant, preds, gates, tgt, w, h, *_weights(c))
        assert bool((prow == -1).all()) and bool((pcol == -1).all()) and bool((dpred[:, :, 2:] == 0).all())


# ------------------------------------------------------------------------------------------------ loss values and gradients
@pytest.mark.parametrize("name,kind", CC.PAIRS)
def test_criterion_vs_fp64_statement(K, name, kind):
    c = CC.BY_NAME[name]
    w, h = c["img"]
    preds, gates, tgt = _dev(name)
    want = CC.integers(name, kind)
    outs = {}
    if kind == "v3":
        loss, dpred, dgate, rows, srt = K.frame_loss(preds, gates, tgt, w, h, *_weights(c), *CC.LIOU)
        assert torch.equal(_cpu(rows), want["rows_by_col"]) and torch.equal(_cpu(srt), want["rows_sorted"])
        M = CC.matchings(name, kind)
        for q in range(6):                                       # QUAD = 1 (inside the loss) against QUAD = 4 (lane_assign)
            r4, s4, _, cost = K.lane_assign(preds[q], tgt, w, h, want_cost=True)
            assert torch.equal(r4, rows[q]) and torch.equal(s4, srt[q])
            if M[q].orig:
                outs[f"cost{q}"] = _cpu(cost)[:, M[q].orig]
        l1, d1, g1, r1, s1 = K.clip_loss([preds], [gates], tgt.unsqueeze(0), w, h, *_weights(c), *CC.LIOU)
        for a, b in ((l1, loss), (d1[0], dpred), (g1[0], dgate), (r1[0], rows), (s1[0], srt)):
            assert torch.equal(a, b), "clip_loss at T = 1 is frame_loss"
    else:
        loss, dpred, dgate, prow, pcol, srt = K.frame_loss_variant(int(kind[1]), preds, gates, tgt, w, h, *_weights(c))
        assert torch.equal(_cpu(prow), want["pair_rows"]), (_cpu(prow), want["pair_rows"])
        assert torch.equal(_cpu(pcol), want["pair_cols"]), (_cpu(pcol), want["pair_cols"])
        if kind == "v1":
            assert torch.equal(_cpu(srt), want["rows_sorted"])
    outs["loss"] = _cpu(loss)
    for q in range(6):
        outs[f"dpred{q}"] = _cpu(dpred[q])
    for q in range(3):
        outs[f"dgate{q}"] = _cpu(dgate[q])
    _judge(name, kind, outs)


def test_clip_loss_at_8_frames_is_8_frame_losses(K):
    """T = MAXT = 8: frames of `w63` with 2, 1 and 0 valid label rows, the six predictions rotated from frame to frame."""
    c = CC.BY_NAME["w63"]
    w, h = c["img"]
    preds, gates, tgt = _dev("w63")
    flags = [(1, 1), (1, 0), (0, 0), (0, 1), (1, 1), (0, 0), (1, 0), (1, 1)]
    fp, fg, ft = [], [], []
    for f, fl in enumerate(flags):
        fp.append([preds[(q + f) % 6] for q in range(6)])
        fg.append([gates[(q + f) % 3] for q in range(3)])
        t = tgt.clone()
        t[:, 1] = torch.tensor(fl, dtype=torch.float32)
        ft.append(t)
    args = (w, h, *_weights(c), *CC.LIOU)
    loss, dpred, dgate, rows, srt = K.clip_loss(fp, fg, torch.stack(ft).contiguous(), *args)
    seen = set()
    for f in range(8):
        one = K.frame_loss(fp[f], fg[f], ft[f], *args)
        for a, b in zip((loss[f:f + 1], dpred[f], dgate[f], rows[f], srt[f]), one):
            assert torch.equal(a, b), f
        seen.add(int((rows[f, 0] >= 0).sum()))
    assert seen == {0, 1, 2}


# ------------------------------------------------------------------------------------------------ writes past the end
def _buf(n, dtype):
    if dtype == torch.float32:
        return torch.full((n + PAD,), F32_SENT, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full((n + PAD,), I64_SENT, dtype=dtype, device="cuda")


def _bits(t):
    return (t.view(torch.int32) if t.dtype == torch.float32 else t).cpu()


def _sent(t):
    return F32_SENT if t.dtype == torch.float32 else I64_SENT


def _written(t, n, what):
    """All of the first n elements written, the PAD behind them untouched."""
    b = _bits(t)
    assert not bool((b[:n] == _sent(t)).any()), (what, "a sentinel is left inside")
    assert bool((b[n:] == _sent(t)).all()), (what, "written past its end")


def _untouched(t, what):
    assert bool((_bits(t) == _sent(t)).all()), (what, "written")


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _clip_buffers(T, N, L, W):
    return dict(loss=_buf(T, torch.float32), dgate=_buf(T * 3 * N, torch.float32), rows=_buf(T * 6 * L, torch.int64),
                srt=_buf(T * 6 * L, torch.int64), focal=_buf(T * 6 * N, torch.float32), scalars=_buf(T * 12, torch.float32),
                dpred=[_buf(N * W, torch.float32) for _ in range(6 * T)])


def _call_clip(lib, st, preds, gates, tgt, b, T, N, L, S, c):
    return lib.phnet_clip_loss(_ptrs(preds), _ptrs(gates), tgt.data_ptr(), T, N, L, S, float(c["img"][0]), float(c["img"][1]), *map(float, _weights(c)),
                               *map(float, CC.LIOU), b["loss"].data_ptr(), _ptrs(b["dpred"]), b["dgate"].data_ptr(), b["rows"].data_ptr(),
                               b["srt"].data_ptr(), b["focal"].data_ptr(), b["scalars"].data_ptr(), st)


def _variant_buffers(N, L, W):
    return dict(loss=_buf(1, torch.float32), dgate=_buf(3 * N, torch.float32), prow=_buf(6 * 16, torch.int64), pcol=_buf(6 * 16, torch.int64),
                srt=_buf(6 * L, torch.int64), scratch=_buf(6 * N + 192, torch.float32), dpred=[_buf(N * W, torch.float32) for _ in range(6)])


def _call_variant(lib, st, variant, preds, gates, tgt, b, N, L, S, c):
    return lib.phnet_frame_loss_variant(variant, _ptrs(preds), _ptrs(gates), tgt.data_ptr(), N, L, S, float(c["img"][0]), float(c["img"][1]),
                                        *map(float, _weights(c)), b["loss"].data_ptr(), _ptrs(b["dpred"]), b["dgate"].data_ptr(),
                                        b["prow"].data_ptr(), b["pcol"].data_ptr(), b["srt"].data_ptr(), b["scratch"].data_ptr(), st)


@pytest.mark.parametrize("name", ["one", "odd", "long"])
def test_nothing_is_written_past_the_end(K, name):
    """phnet_clip_loss (T = 2) and phnet_frame_loss_variant called directly on over-allocated, sentinel-filled outputs: every
    output and scratch buffer is written in full and not beyond.  (rows_sorted is not an output of variant 2: it stays untouched.)"""
    from phnet_amd import _lib
    lib, st = _lib.lib(), K._stream()
    c = CC.BY_NAME[name]
    N, L, S = c["N"], c["L"], c["S"]
    W, T = 6 + S, 2
    preds, gates, tgt = _dev(name)
    b = _clip_buffers(T, N, L, W)
    assert _call_clip(lib, st, preds + preds[::-1], gates * 2, torch.stack([tgt, tgt]).contiguous(), b, T, N, L, S, c) == 0
    torch.cuda.synchronize()
    for k, n in (("loss", T), ("dgate", T * 3 * N), ("rows", T * 6 * L), ("srt", T * 6 * L), ("focal", T * 6 * N), ("scalars", T * 12)):
        _written(b[k], n, k)
    for i, d in enumerate(b["dpred"]):
        _written(d, N * W, f"dpred[{i}]")
    for variant in (1, 2):
        b = _variant_buffers(N, L, W)
        assert _call_variant(lib, st, variant, preds, gates, tgt, b, N, L, S, c) == 0
        torch.cuda.synchronize()
        for k, n in (("loss", 1), ("dgate", 3 * N), ("prow", 96), ("pcol", 96), ("scratch", 6 * N + 192)):
            _written(b[k], n, (variant, k))
        if variant == 1:
            _written(b["srt"], 6 * L, (variant, "rows_sorted"))
        else:
            _untouched(b["srt"], (variant, "rows_sorted"))
        for i, d in enumerate(b["dpred"]):
            _written(d, N * W, (variant, f"dpred[{i}]"))


@pytest.mark.parametrize("what,bad", [("N", 0), ("N", 257), ("L", 5), ("S", 2), ("S", 251), ("T", 0), ("T", 9), ("variant", 3)])
def test_bad_arguments_are_rejected_and_nothing_is_written(K, what, bad):
    from phnet_amd import _lib
    lib, st = _lib.lib(), K._stream()
    c = CC.BY_NAME["few"]
    dims = dict(N=c["N"], L=c["L"], S=c["S"], T=1, variant=1)
    preds, gates, tgt = _dev("few")
    W = 6 + dims["S"]
    dims[what] = bad
    if what != "variant":
        b = _clip_buffers(1, c["N"], c["L"], W)
        assert _call_clip(lib, st, preds, gates, tgt, b, dims["T"], dims["N"], dims["L"], dims["S"], c) == ERR_ARG
        torch.cuda.synchronize()
        for k, v in b.items():
            for t in (v if isinstance(v, list) else [v]):
                _untouched(t, k)
    if what != "T":
        b = _variant_buffers(c["N"], c["L"], W)
        assert _call_variant(lib, st, dims["variant"], preds, gates, tgt, b, dims["N"], dims["L"], dims["S"], c) == ERR_ARG
        torch.cuda.synchronize()
        for k, v in b.items():
            for t in (v if isinstance(v, list) else [v]):
                _untouched(t, k)
