"""The GEMM shapes shared by tests/test_gemm_coverage_cpu.py (which kernel and split count the library picks, no GPU) and
tests/test_gemm_coverage_gpu.py (what those launches compute, against fp64): one row per launch the default tuning
(bf16x3, mma mode 3) must make, found with the library's own host-only phnet_*_kernel queries - no forced tile or split.

A row is (op, shape, kernel, splits, reason):
  op      fwd | dgrad | wgrad | wgrad_dbias | conv3p_fwd | conv3p_dgrad | linear_bwd | linear_bwd_relu
  shape   (N, Hi, Wi, Ci, Co, R, stride, pad) of the convolution (a Linear layer is a 1x1 convolution over an [M,1,1,K] image);
          (N, Hi, Wi, Ci, Co) of the 3x3 / stride 1 / pad 1 convolution for the conv3p ops; (M, K, N) for the linear_bwd ops
  kernel  the symbol the query must answer; splits: the split factor it must answer (None for linear_bwd: one fused launch)
  reason  one word: what this row is the cover of
No torch.cuda here: the module only describes shapes and restates the launch arithmetic."""
import collections

from phnet_amd.hip_ops import splitk_workspace_bytes      # the scratch hip_ops hands a launch with an [m, cols] output (importing it touches no GPU)

Row = collections.namedtuple("Row", "op shape kernel splits reason")

IGEMM = "conv_igemm_kernel<%s>"
T128X128, T128X128_D = IGEMM % "128, 128, false, 16, false, 3, 4, false", IGEMM % "128, 128, true, 16, false, 3, 4, false"
T128X64, T128X64_D = IGEMM % "128, 64, false, 16, false, 3, 4, false", IGEMM % "128, 64, true, 16, false, 3, 4, false"
T64, T64_D = IGEMM % "64, 64, false, 16, true, 3, 4, true", IGEMM % "64, 64, true, 16, true, 3, 4, true"
T64_D_DILATED = IGEMM % "64, 64, true, 16, true, 3, 4, false"           # stride-2 data gradient: no buffer loads
T64_DEEP, T64_DEEP_D = IGEMM % "64, 64, false, 64, true, 3, 4, true", IGEMM % "64, 64, true, 64, true, 3, 4, true"
T64_DEEP_D_RAGGED = IGEMM % "64, 64, true, 64, false, 3, 4, false"      # Co no multiple of the 64-deep K tile: per-thread taps
TAPS3, TAPS3_D = "conv3x3s1_kernel<false>", "conv3x3s1_kernel<true>"
P3_1, P3_2 = "conv3p_kernel<1>", "conv3p_kernel<2>"
W3S, W3, W1S = "wgrad3s_kernel<2>", "conv_wgrad3x3_kernel<4, 16>", "wgrad1s_kernel"
WG64, WG128 = "conv_wgrad_kernel<64, 64, 3, 16, 4, true>", "conv_wgrad_kernel<128, 64, 3, 16, 4, true>"
SMALLP = "linear_wgrad_smallp_kernel<64, 64, 0>"
ROWS1, ROWS2 = "linrows_kernel<false, 1>", "linrows_kernel<false, 2>"                # 160 | 320 x 128 tiles, 16-deep steps
ROWS1_D, ROWS2_D = "linrows_kernel<true, 1>", "linrows_kernel<true, 2>"

ROWS = [
    # ---- 128-row tiles (the 8-clip trunk plans), unsplit: ragged rows and columns, stride-2 data gradient
    Row("fwd", (1, 97, 99, 32, 512, 3, 1, 1), T128X128, 1, "tile128x128"),
    Row("dgrad", (1, 97, 99, 512, 32, 3, 1, 1), T128X128_D, 1, "tile128x128"),
    Row("fwd", (2, 61, 79, 16, 516, 1, 1, 0), T128X128, 1, "ragged128x128"),        # M = 9638, Co = 516: ragged both ways
    Row("fwd", (1, 283, 283, 16, 96, 1, 1, 0), T128X64, 1, "tile128x64"),
    Row("dgrad", (1, 283, 283, 96, 16, 1, 1, 0), T128X64_D, 1, "tile128x64"),
    Row("dgrad", (1, 401, 401, 8, 64, 3, 2, 1), T128X64_D, 1, "dilated128x64"),     # stride 2: the A side is dilated
    # ---- 128x128 tiles with split-K
    Row("fwd", (9100, 1, 1, 784, 516, 1, 1, 0), T128X128, 3, "odd_split"),          # 49 K steps over 3 splits: 17 17 15
    Row("fwd", (1, 149, 257, 128, 128, 3, 1, 1), T128X128, 4, "split128x128"),
    Row("dgrad", (1, 149, 257, 128, 128, 3, 1, 1), T128X128_D, 4, "split128x128"),
    # ---- 64-deep K tile (few rows): 29 K steps over 7 splits of 5 leave split 6 without a K range
    Row("fwd", (240, 1, 1, 1856, 2880, 1, 1, 0), T64_DEEP, 7, "empty_split"),
    Row("fwd", (240, 1, 1, 1856, 2876, 1, 1, 0), T64_DEEP, 7, "empty_split"),       # and a ragged Co
    Row("dgrad", (240, 1, 1, 1856, 2876, 1, 1, 0), T64_DEEP_D_RAGGED, 8, "short_split"),
    Row("dgrad", (240, 1, 1, 192, 128, 1, 1, 0), T64_DEEP_D, 1, "unsplit"),
    # ---- conv3x3s1_kernel: split over (filter row, 16-channel chunk) units
    Row("fwd", (1, 20, 50, 128, 128, 3, 1, 1), TAPS3, 4, "split4"),
    Row("dgrad", (1, 20, 50, 128, 128, 3, 1, 1), TAPS3_D, 4, "split4"),
    Row("fwd", (2, 10, 25, 256, 256, 3, 1, 1), TAPS3, 8, "split8"),
    Row("dgrad", (2, 10, 25, 256, 256, 3, 1, 1), TAPS3_D, 8, "split8"),
    Row("fwd", (1, 240, 240, 16, 64, 3, 1, 1), TAPS3, 1, "unsplit"),                # 900 tiles
    Row("dgrad", (1, 240, 240, 16, 64, 3, 1, 1), TAPS3_D, 1, "unsplit"),            # and 16 of 64 output columns
    Row("fwd", (1, 20, 50, 80, 80, 3, 1, 1), TAPS3, 2, "short_split"),              # 15 units: 8 + 7
    Row("dgrad", (1, 20, 50, 80, 80, 3, 1, 1), TAPS3_D, 2, "short_split"),
    # ---- the production 64x64 tile at every split count the fixture records
    Row("fwd", (1200, 1, 1, 4608, 1040, 1, 1, 0), T64, 4, "split4"),                # 1040 columns: no whole 128-column tiles, so not ROWS1
    Row("fwd", (613, 1, 1, 784, 2556, 1, 1, 0), T64, 3, "odd_split"),
    Row("fwd", (613, 1, 1, 1296, 1600, 1, 1, 0), T64, 5, "odd_split"),
    Row("fwd", (763, 1, 1, 1792, 960, 1, 1, 0), T64, 7, "odd_split"),
    Row("fwd", (320, 1, 1, 2064, 64, 1, 1, 0), T64, 8, "short_split"),              # 129 K steps: 7 x 17 + 10
    Row("dgrad", (613, 1, 1, 3836, 528, 1, 1, 0), T64_D, 2, "short_split"),
    Row("dgrad", (613, 1, 1, 2556, 784, 1, 1, 0), T64_D, 3, "odd_split"),
    Row("dgrad", (613, 1, 1, 1924, 1040, 1, 1, 0), T64_D, 4, "short_split"),        # 65 K steps: 17 17 17 14; 1924 columns: not ROWS1_D
    Row("dgrad", (320, 1, 1, 64, 2064, 1, 1, 0), T64_D, 8, "short_split"),
    Row("dgrad", (3, 40, 40, 512, 64, 3, 2, 1), T64_D_DILATED, 2, "dilated_split"),
    # ---- tall tiles for many-row Linear layers: the smallest shapes of the class (more than 192 workgroups of 160 x 128 outputs)
    Row("fwd", (321, 1, 1, 1024, 2176, 1, 1, 0), ROWS1, 4, "split4"),               # 3 x 17 tiles x 4 splits = 204 workgroups
    Row("dgrad", (321, 1, 1, 2176, 1024, 1, 1, 0), ROWS1_D, 4, "split4"),
    Row("fwd", (321, 1, 1, 1792, 1280, 1, 1, 0), ROWS1, 7, "odd_split"),            # 3 x 10 x 7 = 210 (the fixture's 8-clip 2304 -> 384 plan)
    Row("fwd", (321, 1, 1, 1024, 12416, 1, 1, 0), ROWS2, 1, "unsplit"),             # 2 x 97 tiles = 194 workgroups, ragged rows
    Row("dgrad", (321, 1, 1, 12416, 1024, 1, 1, 0), ROWS2_D, 1, "unsplit"),
    # ---- packed-weight 3x3: the unsplit plans and the 128-column tile (the existing list reaches conv3p_kernel<1> at 3, 6, 8)
    Row("conv3p_fwd", (2, 16, 20, 16, 64), P3_1, 1, "unsplit"),
    Row("conv3p_dgrad", (2, 16, 20, 64, 16), P3_1, 1, "unsplit"),
    Row("conv3p_fwd", (1, 128, 129, 16, 128), P3_2, 1, "unsplit"),
    Row("conv3p_dgrad", (1, 128, 129, 128, 16), P3_2, 1, "unsplit"),
    Row("conv3p_fwd", (1, 128, 129, 64, 128), P3_2, 3, "odd_split"),
    Row("conv3p_dgrad", (1, 128, 129, 128, 64), P3_2, 3, "odd_split"),
    # ---- weight gradients, split over pixels: a short last split for every kernel, an empty one where the planner makes one
    # (391 pixels: 25 steps of 16 over 6 splits of 5 - split 5 starts at step 25; 13 steps of 32 over 6 splits of 3 likewise)
    Row("wgrad", (1, 17, 23, 256, 256, 3, 1, 1), W3S, 5, "short_split"),            # 13 steps of 32: 3 3 3 3 1
    Row("wgrad", (1, 17, 23, 64, 64, 3, 1, 1), W3S, 6, "empty_split"),
    Row("wgrad_dbias", (1, 13, 41, 256, 256, 3, 1, 1), W3, 5, "short_split"),       # 34 steps of 16: 7 7 7 7 6
    Row("wgrad_dbias", (1, 17, 23, 64, 64, 3, 1, 1), W3, 6, "empty_split"),
    Row("wgrad", (1025, 1, 1, 1024, 1024, 1, 1, 0), W1S, 4, "short_split"),         # 65 steps: 17 17 17 14 (a last step of one row)
    Row("wgrad_dbias", (1025, 1, 1, 1024, 1024, 1, 1, 0), W1S, 4, "short_split"),
    Row("wgrad", (257, 1, 1, 128, 4, 1, 1, 0), WG64, 4, "short_split"),             # 17 steps: 5 5 5 2
    Row("wgrad", (1, 17, 23, 16, 16, 1, 1, 0), WG64, 6, "empty_split"),
    Row("wgrad_dbias", (1, 17, 23, 16, 16, 1, 1, 0), WG64, 6, "empty_split"),
    Row("wgrad", (1, 12, 46, 32, 128, 3, 2, 1), WG128, 2, "short_split"),           # 138 pixels, 9 steps: 5 4
    Row("wgrad", (1, 17, 23, 32, 128, 1, 1, 0), WG128, 6, "empty_split"),
    Row("wgrad_dbias", (1, 17, 23, 32, 128, 1, 1, 0), WG128, 6, "empty_split"),
    Row("wgrad", (237, 1, 1, 64, 36, 1, 1, 0), SMALLP, 1, "ragged_rows"),           # one launch, no split: 237 = 14 x 16 + 13 rows
    Row("wgrad_dbias", (237, 1, 1, 64, 36, 1, 1, 0), SMALLP, 1, "ragged_rows"),
    # ---- fused Linear backward (one launch; the query reports no split factor)
    Row("linear_bwd", (237, 128, 384), "linear_bwd_fused_kernel<true, false, 0>", None, "ragged_rows"),
    Row("linear_bwd_relu", (237, 128, 384), "linear_bwd_fused_kernel<true, true, 0>", None, "ragged_rows"),
]


def row_id(row: Row) -> str:
    return f"{row.op}-{'x'.join(str(v) for v in row.shape)}-{row.reason}"


def conv_out_hw(hi, wi, r, stride, pad):
    return (hi + 2 * pad - r) // stride + 1, (wi + 2 * pad - r) // stride + 1


def query_args(lib, op: str, shape) -> dict:
    """The argument dict tests/test_dispatch_cpu.py's query() takes, with the workspace size hip_ops would pass for this shape
    (so the query sees the plan the launch runs).  lib: the loaded library (the weight-gradient workspace is its own answer)."""
    if op in ("linear_bwd", "linear_bwd_relu"):
        m, k, n = shape
        return dict(M=m, K=k, N=n)
    if op in ("conv3p_fwd", "conv3p_dgrad"):
        n, hi, wi, ci, co = shape
        ca, nn = (ci, co) if op == "conv3p_fwd" else (co, ci)
        return dict(M=n * hi * wi, Ca=ca, Nn=nn, ws_bytes=splitk_workspace_bytes(n * hi * wi, nn))
    n, hi, wi, ci, co, r, stride, pad = shape
    args = dict(N=n, Hi=hi, Wi=wi, Ci=ci, Co=co, R=r, S=r, stride=stride, pad=pad)
    ho, wo = conv_out_hw(hi, wi, r, stride, pad)
    if op == "fwd":
        args["ws_bytes"] = splitk_workspace_bytes(n * ho * wo, co)
    elif op == "dgrad":
        args["ws_bytes"] = splitk_workspace_bytes(n * hi * wi, ci)
    else:
        assert op in ("wgrad", "wgrad_dbias"), op
        args["ws_bytes"] = int(lib.phnet_conv2d_wgrad_workspace(n, hi, wi, ci, co, r, r, stride, pad))
    return args


# ---- the launch arithmetic, restated: how a launch cuts its reduction range into `splits` pieces --------------------------
# csrc/conv.hip launch_conv:       ksteps = ceil(K / k_tile),  k_per_split = ceil(ksteps / splits) * k_tile
#                                  conv3x3s1_kernel: units = 3 * (A-side channels / 16), k_per_split = ceil(units / splits)
# csrc/conv3p.hip p3_plan:         units = 3 * (Ca / 16),  units_per_split = ceil(units / splits)
# csrc/conv_wgrad.hip phnet_conv2d_wgrad: steps = ceil(P / pixels per step),  pix_per_split = ceil(steps / splits) * pixels per step
WGRAD_PIXELS_PER_STEP = {W3S: 32, W3: 16, W1S: 16, WG64: 16, WG128: 16}


def reduction_steps(row: Row):
    """Number of steps the row's launch splits (K tiles, units or pixel steps), or None where the kernel never splits."""
    if row.op in ("linear_bwd", "linear_bwd_relu") or row.kernel == SMALLP:
        return None
    if row.op in ("conv3p_fwd", "conv3p_dgrad"):
        _, _, _, ci, co = row.shape
        return 3 * ((ci if row.op == "conv3p_fwd" else co) // 16)
    n, hi, wi, ci, co, r, stride, pad = row.shape
    if row.op in ("fwd", "dgrad"):
        a_channels = ci if row.op == "fwd" else co
        if row.kernel in (TAPS3, TAPS3_D):
            return 3 * (a_channels // 16)
        k_tile = 16 if row.kernel.startswith("linrows_kernel<") else int(row.kernel.split(",")[3])
        return -(-(r * r * a_channels) // k_tile)
    ho, wo = conv_out_hw(hi, wi, r, stride, pad)
    return -(-(n * ho * wo) // WGRAD_PIXELS_PER_STEP[row.kernel])


def split_class(steps: int, splits: int) -> str:
    """'even': every split takes ceil(steps / splits) steps; 'short': the last one takes fewer; 'empty': the last one starts
    at or past the end of the range (it still runs, and must still write zeros to its slice of the partial sums)."""
    per_split = -(-steps // splits)
    last = steps - (splits - 1) * per_split
    return "even" if last == per_split else "short" if last > 0 else "empty"
