"""The tall-tile kernel of the many-row Linear layers (csrc/linrows.hip) on a real MI355X: its forward and data gradient are the
generic kernel's bit for bit - every split count, ragged rows and columns, a reduction that ends inside the producers' ring - and hold
the generic kernel's bound against fp64.  Both sides are hip_ops.conv2d_fwd / conv2d_dgrad on the [M,1,1,K] views: the shapes here are
smaller than the class the default tuning admits, so phnet_tune_force_k_tile(-302) takes the kernel for them and -300 keeps them on the
generic one (which kernel the default tuning picks for which shape: tests/test_dispatch_cpu.py).  Run with -m gpu."""
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


def _fwd(ops, lib, mode, x, w, b, relu):
    """x [m][k], w [n][k] -> [m][n] through hip_ops.conv2d_fwd into a NaN-filled output, under phnet_tune_force_k_tile(mode)."""
    (m, k), n = x.shape, w.shape[0]
    assert lib.phnet_tune_force_k_tile(mode) == 0
    y = torch.full((m, 1, 1, n), float("nan"), device=x.device)
    return ops.conv2d_fwd(x.view(m, 1, 1, k), w.view(n, 1, 1, k), b, 1, 0, relu, out=y).view(m, n).clone()


def _dgrad(ops, lib, mode, dy, w):
    """dy [m][k], w [k][n] -> [m][n] through hip_ops.conv2d_dgrad into a NaN-filled output, under phnet_tune_force_k_tile(mode)."""
    (m, k), n = dy.shape, w.shape[1]
    assert lib.phnet_tune_force_k_tile(mode) == 0
    dx = torch.full((m, 1, 1, n), float("nan"), device=dy.device)
    return ops.conv2d_dgrad(dy.view(m, 1, 1, k), w.view(k, 1, 1, n), (1, 1), 1, 0, out=dx).view(m, n).clone()


GENERIC, ROWS = -300, -302


def _splits_of(ops, lib, m, k, n, dgrad):
    """What phnet_conv2d_kernel names for the Linear layer of m rows, depth k, n columns in the current tuning state."""
    name, sp = ctypes.create_string_buffer(96), ctypes.c_int32(0)
    ci, co = (n, k) if dgrad else (k, n)
    assert lib.phnet_conv2d_kernel(dgrad, m, 1, 1, ci, co, 1, 1, 1, 0, ops.splitk_workspace_bytes(m, n), name, len(name),
                                   ctypes.byref(sp)) == 0
    return name.value.decode(), sp.value


@pytest.mark.parametrize("splits", [1, 2, 3])
def test_forward_and_dgrad_equal_the_generic_kernel(ops, lib, data, splits):
    """torch.equal of two hip_ops.conv2d_fwd / conv2d_dgrad runs that differ only in -300 (the generic 64 x 64 kernel) / -302 (this
    kernel), both reading the same forced split count; with and without bias, with and without ReLU."""
    x, w, b, dy = (data[k].float().cuda() for k in ("x", "w", "b", "dy"))
    assert lib.phnet_tune_force_conv_tile(64, 64, splits) == 0
    tall = 2 if splits == 1 else 1
    for mode, fwd, bwd in ((GENERIC, "conv_igemm_kernel<64, 64, false, 16, true, 3, 4, true>", "conv_igemm_kernel<64, 64, true, 16, true, 3, 4, true>"),
                           (ROWS, f"linrows_kernel<false, {tall}>", f"linrows_kernel<true, {tall}>")):
        assert lib.phnet_tune_force_k_tile(mode) == 0
        assert _splits_of(ops, lib, M, K, N, 0) == (fwd, splits) and _splits_of(ops, lib, M, N, K, 1) == (bwd, splits)
    for bias in (b, None):
        for relu in (False, True):
            want = _fwd(ops, lib, GENERIC, x, w, bias, relu)
            got = _fwd(ops, lib, ROWS, x, w, bias, relu)
            assert torch.equal(got, want), (splits, bias is not None, relu, float((got - want).abs().max()))
    # data gradient: dy [M][N] (depth N = 192: 12 steps), w [N][K] -> dx [M][K] (272 columns: two tiles and a ragged third)
    want = _dgrad(ops, lib, GENERIC, dy, w)
    got = _dgrad(ops, lib, ROWS, dy, w)
    assert torch.equal(got, want), (splits, float((got - want).abs().max()))
    # ... and at the depth of the forward (272: 17 steps) on the transposed weight
    wt = w.t().contiguous()                                  # [K][N]: K "output features", N "input features"
    want = _dgrad(ops, lib, GENERIC, x, wt)
    got = _dgrad(ops, lib, ROWS, x, wt)
    assert torch.equal(got, want), (splits, float((got - want).abs().max()))


def test_single_step_equals_the_generic_kernel(ops, lib, data):
    """M = 33 rows, depth 16: one K step, one split."""
    x, w, b = data["x"][:33, :16].float().cuda().contiguous(), data["w"][:, :16].float().cuda().contiguous(), data["b"].float().cuda()
    assert lib.phnet_tune_force_conv_tile(64, 64, 1) == 0
    assert lib.phnet_tune_force_k_tile(ROWS) == 0
    assert _splits_of(ops, lib, 33, 16, N, 0) == ("linrows_kernel<false, 2>", 1) and _splits_of(ops, lib, 33, 16, K, 1) == ("linrows_kernel<true, 2>", 1)
    assert torch.equal(_fwd(ops, lib, ROWS, x, w, b, True), _fwd(ops, lib, GENERIC, x, w, b, True))
    dy = data["dy"][:33, :16].float().cuda().contiguous()   # depth 16
    wd = data["w"][:16].float().cuda().contiguous()         # [16][K]
    assert torch.equal(_dgrad(ops, lib, ROWS, dy, wd), _dgrad(ops, lib, GENERIC, dy, wd))


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
        assert lib.phnet_tune_force_k_tile(ROWS) == 0
        assert _splits_of(ops, lib, M, K, N, 0)[0].startswith("linrows_kernel<false") and _splits_of(ops, lib, M, N, K, 1)[0].startswith("linrows_kernel<true")
        close(_fwd(ops, lib, ROWS, x.cuda(), w.cuda(), b.cuda(), False), ref_y, f"forward, {splits} split(s)")
        close(_fwd(ops, lib, ROWS, x.cuda(), w.cuda(), b.cuda(), True), torch.relu(ref_y), f"forward + ReLU, {splits} split(s)")
        close(_dgrad(ops, lib, ROWS, dy.cuda(), w.cuda()), ref_dx, f"data gradient, {splits} split(s)")
