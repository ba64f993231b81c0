// Backward of a Linear layer over few rows as ONE launch: data gradient (the implicit-GEMM tile program of conv.hip, igemm_tile.h)
// and weight / bias gradient (the few-rows program of conv_wgrad.hip, smallp_tile.h) in different workgroups of one grid.
//
// Also built here, at the end: the conv_igemm_kernel instantiations of arithmetic modes 0 (f32-input MFMA), 1 and 2 (bf16 splits in
// registers; opt-in through phnet_tune_mma), so that they compile beside conv.hip's mode-3 ones instead of after them.  They sit in
// THIS source because the fused kernel's data-gradient half is the igemm_tile instantiation of four of them (64x64 tile, K-strided
// B, 64-deep K tile, modes 0 / 1): built without them in the translation unit, hipcc lays linear_bwd_fused_kernel<*, false, *> out
// differently and those launches take 3 % longer (240 x 128 x 384: 14.6 -> 15.3 us; profiles/README.md "build").
#include <cstdio>
#include "conv_igemm.h"
#include "smallp_tile.h"
#include "tuning.h"

using namespace igemm;

namespace {

// Backward of a Linear layer over few rows in ONE launch: the first `dgrad_tiles` workgroups compute the data gradient
// dX = dY W (tiles of the implicit-GEMM program, K tile 64, unsplit), the others the weight (and bias) gradient with the
// few-rows program above.  The two are independent - both only read dY - and each occupies a handful of CUs, so sharing a
// launch removes one ~8 us dependent launch per layer (there are ~270 such layers in a step).
// AMASK: dY is the gradient of relu(x w^T + b); ymask is that layer's saved output and both roles apply the ReLU mask while
// they stage dY (no separate relu-backward launch, no masked copy of dY in memory).
template <bool UNI, bool AMASK, int MMA = 0>
__global__ __launch_bounds__(THREADS) void linear_bwd_fused_kernel(
    const float* __restrict__ dY, const float* __restrict__ W, const float* __restrict__ X, const float* __restrict__ ymask,
    float* __restrict__ dX, float* __restrict__ dw, float* __restrict__ dbias,
    ConvShape gd, unsigned dgrad_tiles, int P, int Co, int Ci, int want_bias, int accumulate)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (blockIdx.x < dgrad_tiles)
        igemm_tile<64, 64, true, 64, UNI, AMASK, MMA>(dY, W, nullptr, nullptr, dX, gd, 0, lds, blockIdx.x, dgrad_tiles, 0, ymask);
    else
        smallp_tile<64, 64, AMASK, MMA>(dY, X, dw, dbias, P, Co, Ci, want_bias, accumulate, lds, blockIdx.x - dgrad_tiles,
                                   gridDim.x - dgrad_tiles, ymask);
}

}  // namespace

// ---- fused backward of a Linear layer over few rows ------------------------------------------------------------------
static bool linear_bwd_fusable(long M, long K, long N)
{
    if (!tuning().wgrad_smallp || M < 1 || M > SMALLP_MAX || (K & 3) || (N & 3) || K < 4 || N < 4) return false;
    const long wt = ceil_div64(N, 64) * ceil_div64(K, 64), dt = ceil_div64(M, 64) * ceil_div64(K, 64);
    return wt < tuning().smallp_max_tiles && N <= 640 && dt <= 256;   // dgrad stays unsplit: reduction length N <= 640 (gate MLP: 576)
}

// 1 when phnet_linear_bwd runs (M, K, N) as ONE launch; 0: use phnet_conv2d_dgrad + phnet_conv2d_wgrad instead.
PHNET_API int phnet_linear_bwd_fusable(int64_t M, int64_t K, int64_t N) { return linear_bwd_fusable(M, K, N) ? 1 : 0; }

// linear_bwd_fused_kernel<uni, relu, mma>: what phnet_linear_bwd launches and what linear_bwd_kernel_name spells
struct LinearBwdPick { bool uni, relu; int mma; };

static LinearBwdPick pick_linear_bwd(long N, bool has_relu_mask)
{
    return {N % 64 == 0 && tuning().uniform_tap, has_relu_mask, tuning().mma_mode == 1 ? 1 : 0};
}

static int linear_bwd_kernel_name(const LinearBwdPick& p, char* name, int cap)
{
    return snprintf(name, (size_t)cap, "linear_bwd_fused_kernel<%s, %s, %d>", p.uni ? "true" : "false", p.relu ? "true" : "false", p.mma) < cap
               ? PHNET_OK : PHNET_ERR_ARG;
}

// Host-only query: the kernel instantiation phnet_linear_bwd launches for the same shape.
PHNET_API int phnet_linear_bwd_kernel(int32_t M, int32_t K, int32_t N, int32_t has_relu_mask, char* name, int32_t name_cap)
{
    if (!linear_bwd_fusable(M, K, N) || !name || name_cap < 1) return PHNET_ERR_ARG;
    if (tuning().mma_mode == 4) return PHNET_ERR_ARG;               // the bf16 inference arithmetic is forward-only
    return linear_bwd_kernel_name(pick_linear_bwd(N, has_relu_mask != 0), name, name_cap);
}

// Backward of y = x w^T (+ b) for few rows, one launch: dx [M][K] = dy w;  dw [N][K] and dbias [N] (optional) = dy^T x,
// column sums of dy - overwritten or, with accumulate = 1, added to.  dy [M][N], x [M][K], w [N][K], all row-major.
// relu_y (optional, [M][N]): the layer's saved output when it ended in a ReLU - dy is then masked by relu_y > 0 on the fly.
// Only for shapes with phnet_linear_bwd_fusable(M, K, N) == 1 (PHNET_ERR_ARG otherwise).
PHNET_API int phnet_linear_bwd(const float* dy, const float* x, const float* w, const float* relu_y, float* dx, float* dw,
                               float* dbias, int32_t M, int32_t K, int32_t N, int32_t accumulate, void* stream)
{
    if (!linear_bwd_fusable(M, K, N) || !dy || !x || !w || !dx || !dw) return PHNET_ERR_ARG;
    if (tuning().mma_mode == 4) return PHNET_ERR_ARG;               // the bf16 inference arithmetic is forward-only
    ConvShape g{};
    g.N = M; g.Hi = 1; g.Wi = 1; g.Ci = N;              // A side = dY rows, N channels
    g.Ho = 1; g.Wo = 1; g.Co = K;                       // output = dX
    g.R = 1; g.S = 1; g.stride = 1; g.pad = 0; g.in_dil = 1;
    g.splits = 1;
    g.k_per_split = (int)(ceil_div64(N, 64) * 64);
    const unsigned dt = (unsigned)(ceil_div64(M, 64) * ceil_div64(K, 64)), wt = (unsigned)(ceil_div64(N, 64) * ceil_div64(K, 64));
    const int P16 = (M + 15) & ~15;
    const size_t lds_dgrad = 2 * (size_t)(KContigTile<64, 64>::FLOATS + KStridedTile<64, 64>::FLOATS) * sizeof(float);
    const size_t lds_wgrad = (size_t)P16 * 68 * 2 * sizeof(float);
    const size_t lds = lds_dgrad > lds_wgrad ? lds_dgrad : lds_wgrad;
    static bool attr = false;
    if (!attr && !(attr = phnet_allow_dynamic_lds(
                       {(const void*)linear_bwd_fused_kernel<true, true, 0>, (const void*)linear_bwd_fused_kernel<true, false, 0>,
                        (const void*)linear_bwd_fused_kernel<false, true, 0>, (const void*)linear_bwd_fused_kernel<false, false, 0>,
                        (const void*)linear_bwd_fused_kernel<true, true, 1>, (const void*)linear_bwd_fused_kernel<true, false, 1>,
                        (const void*)linear_bwd_fused_kernel<false, true, 1>, (const void*)linear_bwd_fused_kernel<false, false, 1>},
                       (int)((size_t)SMALLP_MAX * 68 * 2 * sizeof(float)))))
        return PHNET_ERR_LAUNCH;
    hipStream_t st = (hipStream_t)stream;
    const LinearBwdPick p = pick_linear_bwd(N, relu_y != nullptr);
#define PHNET_LAUNCH_BWD_(U_, A_, MMA_)                                                                                 \
    hipLaunchKernelGGL((linear_bwd_fused_kernel<U_, A_, MMA_>), dim3(dt + wt), dim3(THREADS), lds, st, dy, w, x, relu_y, dx, \
                       dw, dbias, g, dt, (int)M, (int)N, (int)K, dbias != nullptr, accumulate)
#define PHNET_LAUNCH_BWD(U_, A_)                                                                                        \
    do {                                                                                                                \
        if (p.mma == 1) PHNET_LAUNCH_BWD_(U_, A_, 1);                                                                   \
        else PHNET_LAUNCH_BWD_(U_, A_, 0);                                                                              \
    } while (0)
    if (p.uni && p.relu) PHNET_LAUNCH_BWD(true, true);
    else if (p.uni) PHNET_LAUNCH_BWD(true, false);
    else if (p.relu) PHNET_LAUNCH_BWD(false, true);
    else PHNET_LAUNCH_BWD(false, false);
#undef PHNET_LAUNCH_BWD
#undef PHNET_LAUNCH_BWD_
    return phnet_launch_status();
}

// ---- conv_igemm_kernel in arithmetic modes 0 / 1 / 2 (the rungs of the ladder in conv_igemm.h that conv.hip leaves out) ----
// no buffer-load rung: pick_conv sets p.buf for mode 3 alone
#define PHNET_LAUNCH_CONV_(DGRAD_, BM_, BN_, BKT_, UNI_)                                                                \
    do {                                                                                                                \
        if (p.mma == 1) PHNET_LAUNCH_CONV____(DGRAD_, BM_, BN_, BKT_, UNI_, 1, 1, false);                               \
        else if (p.mma == 2) PHNET_LAUNCH_CONV____(DGRAD_, BM_, BN_, BKT_, UNI_, 2, 1, false);                          \
        else if (p.pf == 4) PHNET_LAUNCH_CONV____(DGRAD_, BM_, BN_, BKT_, UNI_, 0, 4, false);                           \
        else PHNET_LAUNCH_CONV____(DGRAD_, BM_, BN_, BKT_, UNI_, 0, 1, false);                                          \
    } while (0)

void launch_conv_alt(const ConvPick& p, const ConvLaunch& a)
{
    const ConvShape& g = *static_cast<const ConvShape*>(a.shape);
    if (p.dgrad) PHNET_LAUNCH_CONV_TILES(true);
    else PHNET_LAUNCH_CONV_TILES(false);
}
