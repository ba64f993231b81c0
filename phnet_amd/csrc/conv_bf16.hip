// conv_igemm_kernel in arithmetic mode 4, the bf16 inference arithmetic (include/phnet_hip_tuning.h, igemm.h "MMA = 4"): every
// operand element rounded to bf16 once while its tile is staged, ONE v_mfma_f32_32x32x16_bf16 per 16-deep product, f32 accumulation
// and f32 epilogues.  FORWARD instantiations only - the mode has no backward: phnet_conv2d_dgrad / _wgrad / phnet_linear_bwd return
// PHNET_ERR_ARG in it - for every tile, K-tile depth, ring depth and operand path (buffer loads on the uniform-tap tile) that
// pick_conv (conv.hip) can choose, which are mode 3's.  A source of its own so that it compiles beside conv.hip, not after it.
//
// Roofline: MFMA (bf16 pipe, one MFMA per product: 2.5 PFLOP/s dense) - at one clip the loop is bound by operand latency, not by the
// pipe (igemm_tile.h PF); algorithmic FLOP = 2 * M * Co * K.
#include "conv_igemm.h"

using namespace igemm;

#define PHNET_LAUNCH_CONV___(DGRAD_, BM_, BN_, BKT_, UNI_, PF_)                                                         \
    do {                                                                                                                \
        if (p.buf) PHNET_LAUNCH_CONV____(DGRAD_, BM_, BN_, BKT_, UNI_, 4, PF_, UNI_);                                   \
        else PHNET_LAUNCH_CONV____(DGRAD_, BM_, BN_, BKT_, UNI_, 4, PF_, false);                                        \
    } while (0)
#define PHNET_LAUNCH_CONV_(DGRAD_, BM_, BN_, BKT_, UNI_)                                                                \
    do {                                                                                                                \
        if (p.pf == 4) PHNET_LAUNCH_CONV___(DGRAD_, BM_, BN_, BKT_, UNI_, 4);                                           \
        else if (p.pf == 2) PHNET_LAUNCH_CONV___(DGRAD_, BM_, BN_, BKT_, UNI_, 2);                                      \
        else PHNET_LAUNCH_CONV___(DGRAD_, BM_, BN_, BKT_, UNI_, 1);                                                     \
    } while (0)

void launch_conv_bf16(const ConvPick& p, const ConvLaunch& a)
{
    const ConvShape& g = *static_cast<const ConvShape*>(a.shape);
    PHNET_LAUNCH_CONV_TILES(false);
}
