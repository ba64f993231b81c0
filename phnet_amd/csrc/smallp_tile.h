// The few-rows Linear weight-gradient tile program: linear_wgrad_smallp_kernel (conv_wgrad.hip) and the weight-gradient half of
// linear_bwd_fused_kernel (linear_bwd.hip).  Internal, not part of the C-ABI.
#pragma once
#include "igemm.h"

using namespace igemm;

namespace {

// ---- weight gradient of a Linear layer over few rows (P <= 256: the M = 240 layers of the lane head) ------------------
// dW[Co][Ci] (+)= dY^T X with the WHOLE reduction dimension staged in LDS at once: every global load of the workgroup is
// in flight together (one memory latency instead of one per 16-row step - the generic loop needs ~2 us per step, and
// splitting its 15 steps over workgroups costs a second launch), then 15 x 8 MFMAs back to back.  No split, no reduce:
// the result goes (or accumulates) straight into the gradient arena.  The bias gradient is the column sum of the staged
// dY tile.
constexpr int SMALLP_MAX = 256;
template <int BM, int BN, bool AMASK = false, int MMA = 0>
__device__ __forceinline__ void smallp_tile(
    const float* __restrict__ dY, const float* __restrict__ X, float* __restrict__ dw, float* __restrict__ dbias,
    int P, int Co, int Ci, int want_bias, int accumulate, float* lds, unsigned block, unsigned nblocks,
    const float* __restrict__ ymask = nullptr)
{
    constexpr int TM = BM / 2, TN = BN / 2, FM = TM / 32, FN = TN / 32;
    constexpr int AP = BM + 4, BP = BN + 4;
    constexpr int A_CH = BM / 4, B_CH = BN / 4;                     // float4 chunks per staged row
    constexpr int A_LOADS = SMALLP_MAX * A_CH / THREADS, B_LOADS = SMALLP_MAX * B_CH / THREADS;
    const int P16 = (P + 15) & ~15;
    float* As = lds;
    float* Bs = lds + P16 * AP;
    const int tiles_n = (Ci + BN - 1) / BN;
    const unsigned tile = xcd_remap(block, nblocks);
    const int m0 = (int)(tile / tiles_n) * BM, n0 = (int)(tile % tiles_n) * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * TM, wn = (wave & 1) * TN;

    f32x4 ar[A_LOADS], br[B_LOADS], ay[AMASK ? A_LOADS : 1];
    unsigned am = 0, bm = 0;
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i) {                            // branch-free: masked chunks read element 0
        const int idx = tid + THREADS * i, p = idx / A_CH, m = m0 + (idx - p * A_CH) * 4;
        const bool ok = p < P && m < Co;
        ar[i] = *reinterpret_cast<const f32x4*>(dY + (ok ? (size_t)p * Co + m : 0));
        if (AMASK) ay[i] = *reinterpret_cast<const f32x4*>(ymask + (ok ? (size_t)p * Co + m : 0));
        am |= (unsigned)ok << i;
    }
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i) {
        const int idx = tid + THREADS * i, p = idx / B_CH, n = n0 + (idx - p * B_CH) * 4;
        const bool ok = p < P && n < Ci;
        br[i] = *reinterpret_cast<const f32x4*>(X + (ok ? (size_t)p * Ci + n : 0));
        bm |= (unsigned)ok << i;
    }
    // accumulate mode: the accumulators START from the old gradient values, fetched now so that their (cold, HBM) latency
    // overlaps the staging instead of sitting in a read-modify-write epilogue
    f32x16 acc[FM][FN];
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int n = n0 + wn + j * 32 + frag_col(lane), m = m0 + wm + i * 32 + frag_row(lane, e);
                acc[i][j][e] = (accumulate && n < Ci && m < Co) ? dw[(size_t)m * Ci + n] : 0.f;
            }
    const f32x4 zero{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i) {
        const int idx = tid + THREADS * i, p = idx / A_CH;
        f32x4 v = (am >> i) & 1u ? ar[i] : zero;
        if (AMASK) {
            v.x = ay[i].x > 0.f ? v.x : 0.f; v.y = ay[i].y > 0.f ? v.y : 0.f;
            v.z = ay[i].z > 0.f ? v.z : 0.f; v.w = ay[i].w > 0.f ? v.w : 0.f;
        }
        if (p < P16) *reinterpret_cast<f32x4*>(As + p * AP + (idx - p * A_CH) * 4) = v;
    }
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i) {
        const int idx = tid + THREADS * i, p = idx / B_CH;
        if (p < P16) *reinterpret_cast<f32x4*>(Bs + p * BP + (idx - p * B_CH) * 4) = (bm >> i) & 1u ? br[i] : zero;
    }
    __syncthreads();

    for (int ks = 0; ks < P16 / BK; ++ks) {
        float a[FM][8], b[FN][8];
        read_kstrided<FM, AP>(As + wm, lane, ks, a);
        read_kstrided<FN, BP>(Bs + wn, lane, ks, b);
        mma_any<MMA, FM, FN>(a, b, acc);
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int n = n0 + wn + j * 32 + frag_col(lane);
        if (n >= Ci) continue;
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wm + i * 32 + frag_row(lane, e);
                if (m < Co) dw[(size_t)m * Ci + n] = acc[i][j][e];
            }
    }
    if (want_bias && n0 == 0) {                                      // column sums of the staged dY tile: 4 row groups, then fold
        static_assert(BM == 64, "bias fold assumes 64 columns x 4 row groups");
        const int c = tid & 63, grp = tid >> 6;
        float t = 0.f;
#pragma unroll 4
        for (int p = grp; p < P16; p += 4) t += As[p * AP + c];
        __syncthreads();                                            // every wave is done with the MFMA reads of Bs
        Bs[grp * 64 + c] = t;
        __syncthreads();
        if (tid < 64 && m0 + tid < Co) {
            const float v = (Bs[tid] + Bs[64 + tid]) + (Bs[128 + tid] + Bs[192 + tid]);
            dbias[m0 + tid] = accumulate ? dbias[m0 + tid] + v : v;
        }
    }
}

}  // namespace
