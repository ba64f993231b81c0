"""Shared by tests/test_bf16_cpu.py and tests/test_bf16_gpu.py: the bf16 rounding in numpy, the fp64 reference of a convolution /
Linear layer on rounded operands, and the case tables of the "bf16" inference arithmetic (phnet_tune_mma(4),
include/phnet_hip_tuning.h).

The rule under test: a forward GEMM rounds every element of both operands to bf16 (nearest, ties to even) exactly once; products
of two bf16 values are exact in f32; they are summed in f32 accumulators; bias / addend / ReLU / split-K sums / statistics are f32.
So the reference is the fp64 convolution of the ROUNDED operands, and what is left between it and the kernel is f32 accumulation:
the 2e-5 of tests/test_kernels_gpu.py's f32-input MFMA tests."""
import numpy as np

TOL = 2e-5             # close(..., 2e-5) of tests/test_kernels_gpu.py: |a - b| <= 2e-5 * max(1, max |b|)


def round_bf16(x: np.ndarray) -> np.ndarray:
    """float32 array -> the nearest bf16 value of every element (ties to even), as float32.  NaNs stay NaN (quiet, sign kept);
    values that round past the largest bf16 become inf, as in hardware."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    rounded = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    # a NaN keeps its top 16 bits and gets the quiet bit (adding 0x7FFF could carry a NaN payload into the exponent / sign);
    # the sum above can wrap past 2^32 only for negative NaN patterns, which take this branch
    out = np.where(nan, (u & np.uint32(0xFFFF0000)) | np.uint32(0x00400000), rounded).astype(np.uint32)
    return out.view(np.float32).reshape(x.shape)


def conv_ref64(x, w, bias=None, addend=None, relu=False, stride=1, pad=0, rounded=True):
    """x NHWC [N,Hi,Wi,Ci], w OHWI [Co,R,S,Ci] (float32 numpy) -> fp64 NHWC [N,Ho,Wo,Co] of the convolution of the bf16-rounded
    operands (rounded=False: of the operands as given) + bias + addend, ReLU.  bias / addend enter unrounded: they stay f32."""
    import torch
    import torch.nn.functional as F
    xr, wr = (round_bf16(x), round_bf16(w)) if rounded else (x, w)
    xt = torch.from_numpy(xr).double().permute(0, 3, 1, 2)
    wt = torch.from_numpy(wr).double().permute(0, 3, 1, 2)
    y = F.conv2d(xt, wt, None if bias is None else torch.from_numpy(np.asarray(bias)).double(), stride=stride, padding=pad)
    y = y.permute(0, 2, 3, 1)
    if addend is not None:
        y = y + torch.from_numpy(np.asarray(addend)).double()
    if relu:
        y = y.clamp_min(0)
    return y.contiguous().numpy()


# ---- GPU kernel cases: (name, N, Hi, Wi, Ci, Co, R, stride, pad); a Linear layer is (rows, 1, 1, K, Co, 1, 1, 0) ----
CONV_CASES = [
    ("l1_3x3", 2, 16, 20, 64, 64, 3, 1, 1),
    ("l1_3x3_rows", 1, 10, 26, 64, 64, 3, 1, 1),          # packed tile crossing image rows: M = 260 = two 128-row tiles + 4
    ("l2_3x3_128", 2, 10, 20, 128, 128, 3, 1, 1),         # packed, 128 columns
    ("l2_3x3_s2", 5, 20, 50, 64, 128, 3, 2, 1),
    ("l2_1x1_s2", 2, 20, 50, 64, 128, 1, 2, 0),
    ("l4_3x3_splitk", 1, 10, 25, 512, 512, 3, 1, 1),      # split-K
    ("stem_7x7", 2, 33, 47, 4, 64, 7, 2, 3),              # K = 196, ragged
    ("lat_1x1", 3, 9, 13, 128, 64, 1, 1, 0),
]
LINEAR_CASES = [
    ("lin_ragged_co", 240, 1, 1, 64, 36, 1, 1, 0),
    ("lin_head", 240, 1, 1, 1024, 256, 1, 1, 0),
    # the tall tile, which the dispatch takes on its own only for 1024-deep layers that fill the chip: taken here the way
    # tests/test_linrows_gpu.py reaches it at small shapes, tune_k_tile(-302) = for every Linear launch it can run
    ("lin_tall", 1200, 1, 1, 128, 64, 1, 1, 0),
    # 6 outputs: phnet_amd.functional.linear pads the weight to 8 rows for the library (Co % 4 == 0) and slices the result; run
    # under the DEFAULT dispatch, where the tall tile must not apply (shallow K, no whole 128-column tile): the generic kernel
    ("lin_tall_no", 1200, 1, 1, 64, 6, 1, 1, 0),
    ("lin_few", 7, 1, 1, 128, 4, 1, 1, 0),
]
GPU_CASES = CONV_CASES + LINEAR_CASES
PACKED = ("l1_3x3", "l1_3x3_rows", "l2_3x3_128", "l4_3x3_splitk")      # 3x3 / stride 1 with Ci % 16 == 0 and Co % 64 == 0


def lib_shape(c):
    """(N, Hi, Wi, Ci, Co, R, stride, pad) as the library sees the case: output channels padded to a multiple of 4 (functional.linear)."""
    _, n, hi, wi, ci, co, r, stride, pad = c
    return (n, hi, wi, ci, co + (-co) % 4, r, stride, pad)


def case(name):
    return next(c for c in GPU_CASES if c[0] == name)


def out_hw(hi, wi, r, stride, pad):
    return (hi + 2 * pad - r) // stride + 1, (wi + 2 * pad - r) // stride + 1


def make_operands(c, seed=0, integers=False):
    """(x NHWC, w OHWI, bias, addend) float32 numpy.  Default: unit-variance inputs, weights of variance 1 / K (outputs of unit
    scale).  integers=True: all four integer-valued in [-4, 4] - bf16-exact, every partial sum far below 2^24."""
    _, n, hi, wi, ci, co, r, stride, pad = c
    rng = np.random.default_rng(seed)
    ho, wo = out_hw(hi, wi, r, stride, pad)
    if integers:
        draw = lambda *s: rng.integers(-4, 5, size=s).astype(np.float32)      # noqa: E731
        return draw(n, hi, wi, ci), draw(co, r, r, ci), draw(co), draw(n, ho, wo, co)
    k = r * r * ci
    x = rng.standard_normal((n, hi, wi, ci)).astype(np.float32)
    w = (rng.standard_normal((co, r, r, ci)) / np.sqrt(k)).astype(np.float32)
    return x, w, rng.standard_normal(co).astype(np.float32), rng.standard_normal((n, ho, wo, co)).astype(np.float32)


# ---- every conv shape of the ResNet-18 / ResNet-34 + FPN inference at 320 x 800 (the two trunks differ in block counts only) ----
def trunk_conv_shapes(frames: int, hw=(320, 800), fpn_out=64):
    """[(N, Hi, Wi, Ci, Co, R, stride, pad)] without repeats: stem (3 channels padded to 4), the four stages with their stride-2
    entries and 1x1 downsamples, the FPN's 1x1 laterals on layers 2-4 and its 3x3 output convolutions."""
    h, w = hw
    shapes = [(frames, h, w, 4, 64, 7, 2, 3)]
    h, w = out_hw(h, w, 7, 2, 3)
    h, w = out_hw(h, w, 3, 2, 1)                               # max-pool
    cin, levels = 64, []
    for stage, cout in enumerate((64, 128, 256, 512)):
        if stage:
            shapes += [(frames, h, w, cin, cout, 3, 2, 1), (frames, h, w, cin, cout, 1, 2, 0)]
            h, w = out_hw(h, w, 3, 2, 1)
        shapes.append((frames, h, w, cout, cout, 3, 1, 1))
        cin = cout
        levels.append((h, w, cout))
    for h, w, c in levels[1:]:
        shapes += [(frames, h, w, c, fpn_out, 1, 1, 0), (frames, h, w, fpn_out, fpn_out, 3, 1, 1)]
    return shapes


HEAD_LINEAR_SHAPES = [(rows, 1, 1, k, co, 1, 1, 0) for rows in (240, 1200)
                      for k, co in ((1024, 8192), (4608, 1024), (64, 64), (2304, 576), (64, 256), (256, 64))]


def query_shapes():
    """Every shape the CPU test asks the forward queries about, deduplicated."""
    out = []
    for frames in (1, 5, 160):
        out += trunk_conv_shapes(frames)
    out += HEAD_LINEAR_SHAPES + [lib_shape(c) for c in GPU_CASES]
    return list(dict.fromkeys(out))
