"""The data gradient of a stride-2 convolution through the uniform-tap tile program (csrc/igemm_tile.h, DIL): GEMM rows listed by
parity class of the dX pixel, only the live taps of a tile's classes walked, every split the live K tiles of its range of K
(with the 64-deep K tile a one-tap class leaves a split without any: it must write zeros).

Method of tests/test_gemm_coverage_gpu.py: every case first asserts through the host-only query that its launch IS that
instantiation (conv_igemm_kernel<64, 64, true, K tile, true, mode, ring, false>) with the split count written here, then runs it
plain and with an addend into an output pre-filled with a sentinel (a pixel the row order misses shows) between 256 sentinel
rows, against fp64 conv2d autograd on the CPU at 2e-5 of max(1, max|ref|); split launches run twice on a workspace poisoned
with +-1e30 and must repeat bit for bit.  In "bf16x3" and in "f32".  Run with -m gpu."""
import pytest
import torch

from tests import gemm_cases as G
from tests.test_dispatch_cpu import query
from tests.test_gemm_coverage_gpu import SENTINEL, TOL, conv_reference, guarded, twice_on_poison
from tests.test_kernels_gpu import close, nhwc

pytestmark = pytest.mark.gpu

MODES = {"bf16x3": "3, 4", "f32": "0, 1"}            # arithmetic mode and prefetch ring of the name
NAME = "conv_igemm_kernel<64, 64, true, %d, true, %s, false>"

# (N, Hi, Wi, Ci, Co, R, stride, pad) of the forward convolution, what the case is the cover of, and the (K tile, splits) the
# library picks for its data gradient in each arithmetic (found with phnet_conv2d_kernel on the CPU)
CASES = [
    ((1, 6, 6, 16, 64, 3, 2, 1), "four_classes_in_one_tile", {"bf16x3": (64, 2), "f32": (64, 2)}),              # M = 36
    ((2, 9, 13, 32, 64, 3, 2, 1), "odd_sizes_unequal_classes", {"bf16x3": (64, 2), "f32": (64, 2)}),           # M = 234
    ((1, 16, 20, 36, 64, 3, 2, 1), "ragged_columns", {"bf16x3": (16, 2), "f32": (64, 2)}),                     # 36 of 64 columns
    ((3, 10, 12, 64, 128, 1, 2, 0), "one_by_one_dead_classes", {"bf16x3": (16, 1), "f32": (64, 1)}),
    ((1, 9, 11, 64, 128, 1, 2, 0), "one_by_one_odd_sizes", {"bf16x3": (64, 1), "f32": (64, 1)}),
    ((3, 40, 40, 512, 64, 3, 2, 1), "two_splits", {"bf16x3": (16, 2), "f32": (16, 2)}),                        # gemm_cases "dilated_split"
    ((3, 40, 40, 256, 128, 3, 2, 1), "four_splits", {"bf16x3": (16, 4), "f32": (16, 4)}),                      # 75 x 4 tiles
    ((1, 10, 12, 32, 64, 3, 2, 1), "even_sizes_ragged_rows", {"bf16x3": (64, 2), "f32": (64, 2)}),             # M = 120
]
# the same instantiation on an undilated problem (buffer loads tuned off): rows stay pixels, every tap is walked
UNDILATED = ((1, 9, 13, 32, 64, 3, 1, 1), "undilated_identity", {"bf16x3": (64, 2), "f32": (64, 2)})
# the 32-deep K tile (deep K tiles tuned to 32; default arithmetic only)
DEEP32 = ((2, 9, 13, 32, 64, 3, 2, 1), "k_tile_32", {"bf16x3": (32, 2)})


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from phnet_amd import hip_ops
    return hip_ops


def run_case(ops, lib, case, mode):
    shape, _, picks = case
    n, hi, wi, ci, co, r, stride, pad = shape
    k_tile, splits = picks[mode]
    args = G.query_args(lib, "dgrad", shape)
    assert query(lib, "dgrad", args) == (NAME % (k_tile, MODES[mode]), splits), "the launch is not the uniform-tap dilated one"
    ref = conv_reference(shape)
    wd, gyd, addd = nhwc(ref["w"].float()), nhwc(ref["gy"].float()), nhwc(ref["add_x"].float())
    out, check = guarded((n, hi, wi, ci))

    def run():
        out.fill_(SENTINEL)
        plain = ops.conv2d_dgrad(gyd, wd, (hi, wi), stride, pad, out=out).clone()
        out.fill_(SENTINEL)
        return plain, ops.conv2d_dgrad(gyd, wd, (hi, wi), stride, pad, addend=addd, out=out).clone()
    dx, dxa = twice_on_poison(ops, args["ws_bytes"], splits > 1, run)
    check()
    want = ref["dx"].permute(0, 2, 3, 1)
    print(f"{mode} {shape}: max|dx - ref| {float((dx.cpu().double() - want).abs().max()):.3g}, "
          f"with addend {float((dxa.cpu().double() - want - ref['add_x'].permute(0, 2, 3, 1)).abs().max()):.3g}, "
          f"scale {max(1.0, float(want.abs().max())):.3g}")
    close(dx, want, TOL, "dgrad")
    close(dxa, want + ref["add_x"].permute(0, 2, 3, 1), TOL, "dgrad + addend")
    if r == 1 and stride == 2:                      # pixels off the stride grid have no live tap: exactly 0 / exactly the addend
        dead = torch.ones(hi, wi, dtype=torch.bool, device="cuda")
        dead[::2, ::2] = False
        assert bool((dx[:, dead] == 0).all()), "a pixel without a live tap is not 0"
        assert torch.equal(dxa[:, dead], addd[:, dead]), "a pixel without a live tap is not its addend"


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", CASES, ids=[c[1] for c in CASES])
def test_dilated_dgrad_vs_fp64(ops, case, mode):
    from phnet_amd._lib import lib
    try:
        ops.set_mma_mode(mode)
        run_case(ops, lib(), case, mode)
    finally:
        assert lib().phnet_tune_reset() == 0


@pytest.mark.parametrize("mode", list(MODES))
def test_undilated_problem_through_the_same_instantiation(ops, mode):
    from phnet_amd._lib import lib
    try:
        ops.set_mma_mode(mode)
        assert lib().phnet_tune_force_k_tile(-200) == 0          # buffer loads off
        run_case(ops, lib(), UNDILATED, mode)
    finally:
        assert lib().phnet_tune_reset() == 0


def test_dilated_dgrad_k_tile_32(ops):
    from phnet_amd._lib import lib
    try:
        assert lib().phnet_tune_force_k_tile(-32) == 0           # deep K tiles of the default arithmetic: 32
        run_case(ops, lib(), DEEP32, "bf16x3")
    finally:
        assert lib().phnet_tune_reset() == 0

