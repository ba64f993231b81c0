"""The tall-tile kernel of the many-row Linear layers (csrc/linrows.hip) on a real MI355X: its forward and data gradient are the
generic kernel's bit for bit - every split count, ragged rows and columns, a reduction that ends inside the producers' ring - and hold
the generic kernel's bound against fp64; hip_ops takes it for the production shapes only.  The C-ABI entries are called directly:
the shapes here are smaller than phnet_linrows_applies admits.  Run with -m gpu."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

M, N, K = 337, 192, 272        # rows: no multiple of 16, past one tile at both tile heights (160, 320); one and a half 128-column tiles;
                               # 17 steps of 16: odd, ends inside the ring; 2 splits = 9 + 8 steps (a short last split)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from phnet_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def data():
    """x [M][K], w [N][K], bias [N], dy [M][N] in fp64 on the host (shared, never modified) with the fp64 results."""
    g = torch.Generator().manual_seed(337 + 192 + 272)
    x = torch.randn(M, K, dtype=torch.float64, generator=g)
    w = torch.randn(N, K, dtype=torch.float64, generator=g) / K ** 0.5
    b = torch.randn(N, dtype=torch.float64, generator=g)
    dy = torch.randn(M, N, dtype=torch.float64, generator=g)
    return dict(x=x, w=w, b=b, dy=dy, y=x @ w.t() + b, dx=dy @ w)


@pytest.fixture
def lib(ops):
    from phnet_amd._lib import lib
    handle = lib()
    handle.phnet_tune_reset()
    yield handle
    handle.phnet_tune_reset()


def _need(m, cols):
    return 8 * m * cols * 4 if m * cols < (1 << 23) else 0


def _rows_fwd(ops, lib, x, w, b, relu):
    m, k = x.shape
    n = w.shape[0]
    need = _need(m, n)
    ws = ops.workspace(need, x.device)
    y = torch.full((m, n), float("nan"), device=x.device)
    rc = lib.phnet_linrows_fwd(x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(), y.data_ptr(), m, k, n, int(relu),
                               ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return y


def _rows_dgrad(ops, lib, dy, w):
    m, k = dy.shape
    n = w.shape[1]
    need = _need(m, n)
    ws = ops.workspace(need, dy.device)
    dx = torch.full((m, n), float("nan"), device=dy.device)
    rc = lib.phnet_linrows_dgrad(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), m, k, n, ws.data_ptr(), need,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return dx


def _splits_of(lib, m, k, n, dgrad):
    name, sp = ctypes.create_string_buffer(96), ctypes.c_int32(0)
    assert lib.phnet_linrows_kernel(m, k, n, dgrad, _need(m, n), name, len(name), ctypes.byref(sp)) == 0
    return name.value.decode(), sp.value


@pytest.mark.parametrize("splits", [1, 2, 3])
def test_forward_and_dgrad_equal_the_generic_kernel(ops, lib, data, splits):
    """torch.equal against hip_ops.conv2d_fwd / conv2d_dgrad (the generic 64 x 64 kernel: the shape is outside phnet_linrows_applies),
    both reading the same forced split count; with and without bias, with and without ReLU."""
    x, w, b, dy = (data[k].float().cuda() for k in ("x", "w", "b", "dy"))
    assert lib.phnet_tune_force_conv_tile(64, 64, splits) == 0
    assert not ops.linrows_applies(M, K, N, False) and not ops.linrows_applies(M, N, K, True)
    name_f, sp_f = _splits_of(lib, M, K, N, 0)
    name_d, sp_d = _splits_of(lib, M, N, K, 1)
    tall = 2 if splits == 1 else 1
    assert (name_f, sp_f) == (f"linrows_kernel<false, {tall}>", splits) and (name_d, sp_d) == (f"linrows_kernel<true, {tall}>", splits)
    for bias in (b, None):
        for relu in (False, True):
            want = ops.conv2d_fwd(x.view(M, 1, 1, K), w.view(N, 1, 1, K), bias, 1, 0, relu).view(M, N).clone()
            got = _rows_fwd(ops, lib, x, w, bias, relu)
            assert torch.equal(got, want), (splits, bias is not None, relu, float((got - want).abs().max()))
    # data gradient: dy [M][N] (depth N = 192: 12 steps), w [N][K] -> dx [M][K] (272 columns: two tiles and a ragged third)
    want = ops.conv2d_dgrad(dy.view(M, 1, 1, N), w.view(N, 1, 1, K), (1, 1), 1, 0).view(M, K).clone()
    got = _rows_dgrad(ops, lib, dy, w)
    assert torch.equal(got, want), (splits, float((got - want).abs().max()))
    # ... and at the depth of the forward (272: 17 steps) on the transposed weight
    wt = w.t().contiguous()                                  # [K][N]: K "output features", N "input features"
    want = ops.conv2d_dgrad(x.view(M, 1, 1, K), wt.view(K, 1, 1, N), (1, 1), 1, 0).view(M, N).clone()
    got = _rows_dgrad(ops, lib, x, wt)
    assert torch.equal(got, want), (splits, float((got - want).abs().max()))


def test_single_step_equals_the_generic_kernel(ops, lib, data):
    """M = 33 rows, depth 16: one K step, one split."""
    x, w, b = data["x"][:33, :16].float().cuda().contiguous(), data["w"][:, :16].float().cuda().contiguous(), data["b"].float().cuda()
    assert lib.phnet_tune_force_conv_tile(64, 64, 1) == 0
    want = ops.conv2d_fwd(x.view(33, 1, 1, 16), w.view(N, 1, 1, 16), b, 1, 0, True).view(33, N).clone()
    assert torch.equal(_rows_fwd(ops, lib, x, w, b, True), want)
    dy = data["dy"][:33, :16].float().cuda().contiguous()   # depth 16
    wd = data["w"][:16].float().cuda().contiguous()         # [16][K]
    want = ops.conv2d_dgrad(dy.view(33, 1, 1, 16), wd.view(16, 1, 1, K), (1, 1), 1, 0).view(33, K).clone()
    assert torch.equal(_rows_dgrad(ops, lib, dy, wd), want)


def test_against_fp64(ops, lib, data):
    """The bound of test_conv_fwd_dgrad_wgrad_bf16x3 (tests/test_kernels_gpu.py): 2e-5 of the output scale max(1, max |reference|)."""
    def close(a, ref, what):
        a, ref = a.cpu().double(), ref.double()
        scale, err = max(1.0, float(ref.abs().max())), float((a - ref).abs().max())
        print(f"{what}: max error {err:.3e}, scale {scale:.3f}")
        assert err <= 2e-5 * scale, (what, err, scale)

    x, w, b, dy = (data[k].float() for k in ("x", "w", "b", "dy"))
    ref_y = x.double() @ w.double().t() + b.double()
    ref_dx = dy.double() @ w.double()
    for splits in (1, 3):
        assert lib.phnet_tune_force_conv_tile(64, 64, splits) == 0
        close(_rows_fwd(ops, lib, x.cuda(), w.cuda(), b.cuda(), False), ref_y, f"forward, {splits} split(s)")
        close(_rows_fwd(ops, lib, x.cuda(), w.cuda(), b.cuda(), True), torch.relu(ref_y), f"forward + ReLU, {splits} split(s)")
        close(_rows_dgrad(ops, lib, dy.cuda(), w.cuda()), ref_dx, f"data gradient, {splits} split(s)")


PRODUCTION = [(1200, 1024, 8192, 0), (1200, 8192, 1024, 1), (1200, 4608, 1024, 0)]          # M, depth, columns, dgrad


def test_dispatch(ops, lib):
    """phnet_linrows_applies holds for the three production shapes with their split counts 1, 4, 4 and not for few rows, a depth
    that is no multiple of 16 or another arithmetic; with the switch off hip_ops.linear_fwd names the generic symbol.  Host-side
    queries only: nothing launches."""
    for (m, k, n, dgrad), splits in zip(PRODUCTION, (1, 4, 4)):
        assert lib.phnet_linrows_applies(m, k, n, dgrad) == 1, (m, k, n, dgrad)
        name, sp = _splits_of(lib, m, k, n, dgrad)
        assert sp == splits and name == f"linrows_kernel<{'true' if dgrad else 'false'}, {2 if splits == 1 else 1}>", (name, sp)
    assert lib.phnet_linrows_applies(240, 1024, 8192, 0) == 0
    assert lib.phnet_linrows_applies(256, 1024, 8192, 0) == 0
    assert lib.phnet_linrows_applies(1200, 1000, 8192, 0) == 0
    assert lib.phnet_tune_mma(0) == 0
    assert all(lib.phnet_linrows_applies(m, k, n, d) == 0 for m, k, n, d in PRODUCTION)
    lib.phnet_tune_reset()
    assert lib.phnet_tune_force_k_tile(-300) == 0
    assert all(lib.phnet_linrows_applies(m, k, n, d) == 0 for m, k, n, d in PRODUCTION)
    # what hip_ops.linear_fwd records for the timer with the switch off / on (the symbol query, not a launch)
    seen = []
    saved = ops._timed_launch
    ops._timed_launch = lambda sym_fn, flops, launch, **kw: seen.append(sym_fn())
    try:
        x, w = torch.empty(1200, 1024, device="cuda"), torch.empty(8192, 1024, device="cuda")
        ops.linear_fwd(x, w, None)
        assert lib.phnet_tune_force_k_tile(-301) == 0
        ops.linear_fwd(x, w, None)
    finally:
        ops._timed_launch = saved
    assert seen == [("conv_igemm_kernel<64, 64, false, 16, true, 3, 4, true>", 1), ("linrows_kernel<false, 2>", 1)], seen
