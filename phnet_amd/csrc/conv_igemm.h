// conv_igemm_kernel and the macro ladder that launches it: what conv.hip (arithmetic mode 3), linear_bwd.hip (modes 0 / 1 / 2) and
// conv_bf16.hip (mode 4, forward only) share.  The instantiations are split over two sources only because they are the slowest thing in the build; the decision
// (pick_conv), the name (conv_kernel_name) and the launch arithmetic (launch_conv) stay in conv.hip.  Internal, not part of the C-ABI.
#pragma once
#include "igemm_tile.h"

namespace {

template <int BM, int BN, bool B_DGRAD, int BKT, bool UNI, int MMA = 0, int PF = 1, bool BUF = false>
__global__ __launch_bounds__(THREADS) void conv_igemm_kernel(
    const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias,
    const float* __restrict__ addend, float* __restrict__ out, ConvShape g, int relu, float* __restrict__ stats)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // The uniform-tap data gradient without buffer loads is the one that meets dilated dY images (stride-2 convolutions): those run
    // igemm_tile's DIL form, every other problem the plain one - the instantiation linear_bwd_fused_kernel shares (linear_bwd.hip).
    if constexpr (B_DGRAD && UNI && !BUF) {
        if (g.in_dil == 2 && g.R <= 16 && g.S <= 16 && g.R * g.S <= 16) {
            igemm_tile<BM, BN, B_DGRAD, BKT, UNI, false, MMA, PF, BUF, true>(X, W, bias, addend, out, g, relu, lds, blockIdx.x, gridDim.x,
                                                                             blockIdx.z, nullptr, stats);
            return;
        }
    }
    igemm_tile<BM, BN, B_DGRAD, BKT, UNI, false, MMA, PF, BUF>(X, W, bias, addend, out, g, relu, lds, blockIdx.x, gridDim.x, blockIdx.z,
                                                               nullptr, stats);
}

}  // namespace

// What one forward / data-gradient call launches.  Decided once (pick_conv); launch_conv launches it, conv_kernel_name spells it.
struct ConvPick {
    bool taps3;                          // conv3x3s1_kernel<dgrad>; else conv_igemm_kernel<bm, bn, dgrad, bkt, uni, mma, pf, buf>
    int rows;                            // 1 | 2: linrows_kernel<dgrad, rows> (linrows.hip) on bm x bn = 160 * rows x 128 tiles of 16-deep steps;
                                         // bkt is still the K tile whose multiples the splits take, as in the generic kernel
    bool dgrad, uni, buf;
    int bm, bn, bkt, mma, pf, splits;
    long tiles;
};

// One conv_igemm_kernel launch as launch_conv has laid it out.  shape: the ConvShape (splits and k_per_split set) - by address,
// because the type lives in the unnamed namespace and this struct crosses translation units.
struct ConvLaunch {
    const float *X, *W, *bias, *addend;
    float *dst, *stats;                  // dst: the output or the split-K partial sums; stats: null when split
    const void* shape;
    int relu;
    dim3 grid;
    hipStream_t st;
};

// linear_bwd.hip: the launch for p.mma 0 / 1 / 2
void launch_conv_alt(const ConvPick& p, const ConvLaunch& a);
// conv_bf16.hip: the launch for p.mma == 4 (bf16 inference arithmetic: forward only, p.dgrad is false)
void launch_conv_bf16(const ConvPick& p, const ConvLaunch& a);

// The ladder from a pick to its instantiation, for a function that has p (ConvPick), a (ConvLaunch) and g (ConvShape) in scope.
// The including source defines the arithmetic rungs it builds: PHNET_LAUNCH_CONV_(DGRAD_, BM_, BN_, BKT_, UNI_).
#define PHNET_LAUNCH_CONV____(DGRAD_, BM_, BN_, BKT_, UNI_, MMA_, PF_, BUF_)                                            \
    do {                                                                                                                \
        constexpr int np_ = MMA_ == 4 ? 1 : 3;                                                                          \
        constexpr size_t lds_ = (MMA_ == 3 || MMA_ == 4)                                                                \
            ? 2 * (size_t)(KContigPlanes<BM_, BKT_, np_>::BYTES +                                                       \
                           (DGRAD_ ? KStridedPlanes<BN_, BKT_, np_>::BYTES : KContigPlanes<BN_, BKT_, np_>::BYTES))     \
            : 2 * (size_t)(KContigTile<BM_, BKT_>::FLOATS +                                                             \
                           (DGRAD_ ? KStridedTile<BN_, BKT_>::FLOATS : KContigTile<BN_, BKT_>::FLOATS)) * 4;            \
        static bool attr_set_ = false;                                                                                  \
        if (lds_ > 64 * 1024 && !attr_set_) {                                                                           \
            (void)hipFuncSetAttribute((const void*)conv_igemm_kernel<BM_, BN_, DGRAD_, BKT_, UNI_, MMA_, PF_, BUF_>,    \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_);                                 \
            attr_set_ = true;                                                                                           \
        }                                                                                                               \
        hipLaunchKernelGGL((conv_igemm_kernel<BM_, BN_, DGRAD_, BKT_, UNI_, MMA_, PF_, BUF_>), a.grid, dim3(THREADS), lds_, a.st, \
                           a.X, a.W, a.bias, a.addend, a.dst, g, a.relu, a.stats);                                      \
    } while (0)
#define PHNET_LAUNCH_CONV(DGRAD_, BM_, BN_, UNI_)                                                                       \
    do {                                                                                                                \
        if (p.bkt == 64) PHNET_LAUNCH_CONV_(DGRAD_, BM_, BN_, 64, UNI_);                                                \
        else if (p.bkt == 32) PHNET_LAUNCH_CONV_(DGRAD_, BM_, BN_, 32, UNI_);                                           \
        else PHNET_LAUNCH_CONV_(DGRAD_, BM_, BN_, 16, UNI_);                                                            \
    } while (0)
#define PHNET_LAUNCH_CONV_TILES(DGRAD_)                                                                                 \
    do {                                                                                                                \
        if (p.bm == 128 && p.bn == 128) PHNET_LAUNCH_CONV(DGRAD_, 128, 128, false);                                     \
        else if (p.bm == 128 && p.bn == 64) PHNET_LAUNCH_CONV(DGRAD_, 128, 64, false);                                  \
        else if (p.bm == 64 && p.bn == 128) PHNET_LAUNCH_CONV(DGRAD_, 64, 128, false);                                  \
        else if (p.uni) PHNET_LAUNCH_CONV(DGRAD_, 64, 64, true);                                                        \
        else PHNET_LAUNCH_CONV(DGRAD_, 64, 64, false);                                                                  \
    } while (0)
