"""The label-assignment kernels against the bits recorded from the parent build (tests/golden/assign_parent_bits.npz, written by
tests/golden/make_goldens_assign_bits.py on the MI355X): cost matrix, matched rows, tokens and one-to-many pairs must come out
identical, bit for bit, and nothing may be written outside [L], [N*L], [(L+1)*E], [L+1], [16].  The C entry points are called
directly so that every output buffer can be over-allocated and pre-filled with a sentinel.  Run with -m gpu."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_goldens_assign_bits", os.path.join(HERE, "golden", "make_goldens_assign_bits.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
FIXTURE = G.load()
PAD = 64                       # elements behind every output
I64_SENT, I32_SENT, U8_SENT, F32_SENT = -7777, -7777, 0x5A, 0x7FC12345        # the float sentinel is a NaN with a payload of its own


def _id(i):
    c = FIXTURE[i][0]
    return f"{i}-N{c['N']}-L{c['L']}-S{c['S']}-E{c['E']}-v{''.join(map(str, c['valid']))}" + (f"-{c['off']}" if c["off"] else "") + (f"-{c['dup']}" if c["dup"] else "")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from phnet_amd import _lib
    return _lib.lib()


def _buf(n, dtype, sent):
    if dtype == torch.float32:
        return torch.full((n + PAD,), sent, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full((n + PAD,), sent, dtype=dtype, device="cuda")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _expect(t, n, want, sent, what):
    """The first n elements are the recorded bits, the PAD behind them still hold the sentinel."""
    want = torch.from_numpy(np.ascontiguousarray(want).reshape(-1))
    if want.dtype == torch.uint32:
        want = want.view(torch.int32)
    got = _bits(t).cpu()
    assert torch.equal(got[:n], want.to(got.dtype)), (what, "differs from the parent's bits")
    assert torch.equal(got[n:], torch.full((PAD,), sent, dtype=got.dtype)), (what, "written past its end")


@pytest.mark.parametrize("i", range(len(FIXTURE)), ids=_id)
def test_assignment_is_the_parents_bit_for_bit(lib, i):
    from phnet_amd import hip_ops as K
    from phnet_amd._lib import check
    c, rec = FIXTURE[i]
    N, L, S, E = c["N"], c["L"], c["S"], c["E"]
    pred, tgt, feat = (torch.from_numpy(a).cuda() for a in G.case_inputs(c))
    w, h, st = float(G.IMG_W), float(G.IMG_H), K._stream()

    rows, srt, nv, cost = _buf(L, torch.int64, I64_SENT), _buf(L, torch.int64, I64_SENT), _buf(1, torch.int32, I32_SENT), _buf(N * L, torch.float32, F32_SENT)
    check(lib.phnet_lane_assign(pred.data_ptr(), tgt.data_ptr(), N, L, S, w, h, rows.data_ptr(), srt.data_ptr(), nv.data_ptr(), cost.data_ptr(), st), "lane_assign")
    _expect(cost, N * L, rec["cost"], F32_SENT, "cost")
    _expect(rows, L, rec["rows_by_col"], I64_SENT, "rows_by_col")
    _expect(srt, L, rec["rows_sorted"], I64_SENT, "rows_sorted")
    _expect(nv, 1, rec["n_valid"], I32_SENT, "n_valid")

    rows, srt = _buf(L, torch.int64, I64_SENT), _buf(L, torch.int64, I64_SENT)
    tokens, valid = _buf((L + 1) * E, torch.float32, F32_SENT), _buf(L + 1, torch.uint8, U8_SENT)
    check(lib.phnet_lane_assign_tokens(pred.data_ptr(), tgt.data_ptr(), N, L, S, w, h, rows.data_ptr(), srt.data_ptr(), feat.data_ptr(), E,
                                       tokens.data_ptr(), valid.data_ptr(), st), "lane_assign_tokens")
    _expect(tokens, (L + 1) * E, rec["tokens"], F32_SENT, "tokens")
    _expect(valid, L + 1, rec["valid"], U8_SENT, "valid")
    _expect(srt, L, rec["tok_rows_sorted"], I64_SENT, "rows_sorted of lane_assign_tokens")
    _expect(rows, L, rec["rows_by_col"], I64_SENT, "rows_by_col of lane_assign_tokens")

    mrows, mcols, mn = _buf(16, torch.int64, I64_SENT), _buf(16, torch.int64, I64_SENT), _buf(1, torch.int32, I32_SENT)
    check(lib.phnet_lane_assign_one2many(pred.data_ptr(), tgt.data_ptr(), N, L, S, w, h, mrows.data_ptr(), mcols.data_ptr(), mn.data_ptr(), st), "one2many")
    _expect(mrows, 16, rec["many_rows"], I64_SENT, "one-to-many rows")
    _expect(mcols, 16, rec["many_cols"], I64_SENT, "one-to-many cols")
    _expect(mn, 1, rec["many_n"], I32_SENT, "one-to-many n")
