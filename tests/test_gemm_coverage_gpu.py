"""Every row of tests/gemm_cases.py on a real MI355X, in the default arithmetic (bf16x3): the launch the library picks for the
row - asserted through the host-only query - against torch.nn.functional.conv2d and its autograd in fp64 on the CPU, at the
tolerance test_conv_fwd_dgrad_wgrad_bf16x3 holds this arithmetic to (2e-5 of max(1, max|ref|)).

Forward and data-gradient rows write into a tensor with sentinel rows in front of and behind the real [M, Co] extent (an edge
tile that writes out of range shows without a fault).  Split rows run twice on a poisoned split-K workspace (a split that
leaves its slice of the partial sums unwritten - an empty last split must write zeros - shows in the sum) and must repeat
bit for bit.  Run with -m gpu."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_cases as G
from tests.test_dispatch_cpu import query
from tests.test_kernels_gpu import close, dev, nhwc

pytestmark = pytest.mark.gpu

TOL = 2e-5
SENTINEL = 12345.0
POISON = (1e30, -1e30)               # large, finite: one unwritten element of the partial sums moves the result by 1e30


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from phnet_amd import hip_ops
    assert hip_ops.mma_mode() == 3, "these rows are the picks of the default arithmetic"
    return hip_ops


def rounded(*shape):
    """fp64 values that are exactly representable in fp32: the device and the reference see the same numbers."""
    return torch.randn(*shape, dtype=torch.float64).float().double()


@functools.lru_cache(maxsize=2)              # rows of one shape are neighbours in the table
def conv_reference(shape):
    """fp64 conv2d and its autograd on the CPU for (N, Hi, Wi, Ci, Co, R, stride, pad); NCHW tensors, computed once per shape."""
    n, hi, wi, ci, co, r, stride, pad = shape
    torch.manual_seed(sum(shape) + 23)
    x = rounded(n, ci, hi, wi).requires_grad_(True)
    w = (torch.randn(co, ci, r, r, dtype=torch.float64) / (ci * r * r) ** 0.5).float().double().requires_grad_(True)
    b = rounded(co)
    y = F.conv2d(x, w, None, stride=stride, padding=pad)
    gy = rounded(*y.shape)
    y.backward(gy)
    return dict(x=x.detach(), w=w.detach(), b=b, y=y.detach(), gy=gy, dx=x.grad, dw=w.grad, add_y=rounded(*y.shape),
                add_x=rounded(*x.shape), dw0=rounded(*w.shape), db0=rounded(co))


def poison_workspace(ops, nbytes, value):
    """Fills the scratch buffer the next launch of this size gets (hip_ops.workspace, slot 0 of the current device)."""
    if nbytes:
        device = torch.device("cuda", torch.cuda.current_device())
        before = ops.workspace(nbytes, device)
        before.view(torch.float32).fill_(value)
        return lambda: ops.workspace(nbytes, device).data_ptr() == before.data_ptr()
    return lambda: True


def guarded(shape):
    """(view of `shape` inside a larger buffer, check): 256 rows of SENTINEL on either side of the view."""
    rows, cols = shape[0] * shape[1] * shape[2], shape[3]
    guard = 256 * cols
    buf = torch.full((guard + rows * cols + guard,), SENTINEL, device="cuda")
    view = buf[guard:guard + rows * cols].view(shape)

    def check():
        assert bool((buf[:guard] == SENTINEL).all()), "wrote in front of the output"
        assert bool((buf[guard + rows * cols:] == SENTINEL).all()), "wrote past the output's M x Co extent"
    return view, check


def twice_on_poison(ops, ws_bytes, split, run):
    """run() on a poisoned workspace; split launches once more on another poison, and the outputs must be bit-equal."""
    same_buffer = poison_workspace(ops, ws_bytes, POISON[0])
    first = [t.clone() for t in run()]
    assert same_buffer(), "the launch ran on another workspace than the poisoned one"
    if split:
        assert ws_bytes > 0
        poison_workspace(ops, ws_bytes, POISON[1])
        for a, b in zip(first, run()):
            assert torch.equal(a, b), "a repeated launch differs"
    return first


def run_conv(ops, lib, row):
    n, hi, wi, ci, co, r, stride, pad = row.shape
    ref = conv_reference(row.shape)
    ws_bytes = G.query_args(lib, row.op, row.shape)["ws_bytes"]
    split = row.splits > 1
    nhwc_ref = lambda t: t.permute(0, 2, 3, 1)                    # noqa: E731
    xd, wd, gyd = nhwc(ref["x"].float()), nhwc(ref["w"].float()), nhwc(ref["gy"].float())
    if row.op == "fwd":
        bd, addd = dev(ref["b"].float()), nhwc(ref["add_y"].float())
        want = ref["y"] + ref["b"].view(1, -1, 1, 1)
        out, check = guarded((n,) + tuple(ref["y"].shape[2:]) + (co,))

        def run():
            return (ops.conv2d_fwd(xd, wd, bd, stride, pad, out=out).clone(),
                    ops.conv2d_fwd(xd, wd, bd, stride, pad, relu=True, out=out).clone(),
                    ops.conv2d_fwd(xd, wd, bd, stride, pad, relu=True, addend=addd, out=out).clone())
        y, yr, ya = twice_on_poison(ops, ws_bytes, split, run)
        check()
        close(y, nhwc_ref(want), TOL, "fwd + bias")
        close(yr, nhwc_ref(F.relu(want)), TOL, "fwd + bias, relu")
        close(ya, nhwc_ref(F.relu(want + ref["add_y"])), TOL, "fwd + bias + addend, relu")
    elif row.op == "dgrad":
        addd = nhwc(ref["add_x"].float())
        out, check = guarded((n, hi, wi, ci))

        def run():
            return (ops.conv2d_dgrad(gyd, wd, (hi, wi), stride, pad, out=out).clone(),
                    ops.conv2d_dgrad(gyd, wd, (hi, wi), stride, pad, addend=addd, out=out).clone())
        dx, dxa = twice_on_poison(ops, ws_bytes, split, run)
        check()
        close(dx, nhwc_ref(ref["dx"]), TOL, "dgrad")
        close(dxa, nhwc_ref(ref["dx"] + ref["add_x"]), TOL, "dgrad + addend")
    else:
        with_bias = row.op == "wgrad_dbias"
        want_db = ref["gy"].sum(dim=(0, 2, 3))

        def run():
            db = torch.full((co,), 7.0, device="cuda") if with_bias else None
            dw = ops.conv2d_wgrad(gyd, xd, wd.shape, stride, pad, dbias=db)
            acc, acc_b = nhwc(ref["dw0"].float()), dev(ref["db0"].float()) if with_bias else None
            ops.conv2d_wgrad(gyd, xd, wd.shape, stride, pad, dw=acc, accumulate=True, dbias=acc_b)
            return (dw, acc) + ((db, acc_b) if with_bias else ())
        got = twice_on_poison(ops, ws_bytes, split, run)
        close(got[0], nhwc_ref(ref["dw"]), TOL, "wgrad")
        close(got[1], nhwc_ref(ref["dw0"] + ref["dw"]), TOL, "wgrad, accumulate")
        if with_bias:
            close(got[2], want_db, TOL, "dbias")
            close(got[3], ref["db0"] + want_db, TOL, "dbias, accumulate")


def run_conv3p(ops, lib, row):
    n, hi, wi, ci, co = row.shape
    ref = conv_reference(row.shape + (3, 1, 1))
    dgrad = row.op == "conv3p_dgrad"
    ca, nn = (co, ci) if dgrad else (ci, co)
    assert ops.conv3p_applies(n * hi * wi, ca, nn)
    ws_bytes = G.query_args(lib, row.op, row.shape)["ws_bytes"]
    nhwc_ref = lambda t: t.permute(0, 2, 3, 1)                    # noqa: E731
    packed = ops.conv3p_pack(nhwc(ref["w"].float()), dgrad)
    if not dgrad:
        xd, bd, addd = nhwc(ref["x"].float()), dev(ref["b"].float()), nhwc(ref["add_y"].float())

        def run():
            return ops.conv3p(xd, packed, nn), ops.conv3p(xd, packed, nn, bias=bd, addend=addd, relu=True)
        y, ya = twice_on_poison(ops, ws_bytes, row.splits > 1, run)
        close(y, nhwc_ref(ref["y"]), TOL, "conv3p")
        close(ya, nhwc_ref(F.relu(ref["y"] + ref["b"].view(1, -1, 1, 1) + ref["add_y"])), TOL, "conv3p + bias + addend, relu")
    else:
        gyd, addd = nhwc(ref["gy"].float()), nhwc(ref["add_x"].float())

        def run():
            return ops.conv3p(gyd, packed, nn, dgrad=True), ops.conv3p(gyd, packed, nn, dgrad=True, addend=addd)
        dx, dxa = twice_on_poison(ops, ws_bytes, row.splits > 1, run)
        close(dx, nhwc_ref(ref["dx"]), TOL, "conv3p dgrad")
        close(dxa, nhwc_ref(ref["dx"] + ref["add_x"]), TOL, "conv3p dgrad + addend")


def run_linear_bwd(ops, row):
    m, k, n = row.shape
    assert ops.linear_bwd_fusable(m, k, n)
    torch.manual_seed(m + k + n + 23)
    x, dy, dw0, db0 = rounded(m, k), rounded(m, n), rounded(n, k), rounded(n)
    w = (torch.randn(n, k, dtype=torch.float64) / k ** 0.5).float().double()
    relu_y = torch.relu(rounded(m, n)) if row.op == "linear_bwd_relu" else None
    g = dy if relu_y is None else dy * (relu_y > 0)
    xd, dyd, wd = dev(x.float()), dev(dy.float()), dev(w.float())
    yd = None if relu_y is None else dev(relu_y.float())
    dw, db = torch.empty(n, k, device="cuda"), torch.empty(n, device="cuda")
    dx = ops.linear_bwd(dyd, xd, wd, dw, db, accumulate=False, relu_y=yd)
    close(dx, g @ w, TOL, "dx"); close(dw, g.t() @ x, TOL, "dw"); close(db, g.sum(0), TOL, "dbias")
    acc, acc_b = dev(dw0.float()), dev(db0.float())
    dx2 = ops.linear_bwd(dyd, xd, wd, acc, acc_b, accumulate=True, relu_y=yd)
    assert torch.equal(dx2, dx)
    close(acc, dw0 + g.t() @ x, TOL, "dw, accumulate"); close(acc_b, db0 + g.sum(0), TOL, "dbias, accumulate")


@pytest.mark.parametrize("row", G.ROWS, ids=G.row_id)
def test_production_launch_vs_fp64(ops, row):
    from phnet_amd._lib import lib
    assert query(lib(), row.op, G.query_args(lib(), row.op, row.shape)) == (row.kernel, row.splits)
    if row.op in ("linear_bwd", "linear_bwd_relu"):
        run_linear_bwd(ops, row)
    elif row.op in ("conv3p_fwd", "conv3p_dgrad"):
        run_conv3p(ops, lib(), row)
    else:
        run_conv(ops, lib(), row)
