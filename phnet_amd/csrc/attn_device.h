// The per-(query row, head) body of the attention forward for heads of width 16 (gfx950), shared by attn_fwd_kernel
// (attention.hip) and the cross-attention stage of rowchain_attn_kernel (rowchain.hip): both run the same rows through the same
// instructions, so a pass through either gives the same bits.
#pragma once
#include "common.h"

namespace attn_dev {

constexpr int D = 16;                 // head width
constexpr int LPR = 16;               // lanes per row: each walks every 16th key (or query) - the per-lane loop is the critical path
typedef float f4 __attribute__((ext_vector_type(4)));

// 16-wide dot products with four independent partial sums (a single chain of 16 dependent FMAs is pure latency here)
__device__ __forceinline__ float dot16(const float (&a)[D], const float* b) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int d = 0; d < D; d += 4) { s0 += a[d] * b[d]; s1 += a[d + 1] * b[d + 1]; s2 += a[d + 2] * b[d + 2]; s3 += a[d + 3] * b[d + 3]; }
    return (s0 + s1) + (s2 + s3);
}

// LPR adjacent lanes -> one row: reduce across them
__device__ __forceinline__ float quad_sum(float v) {
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float quad_max(float v) {
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// the 16 floats of one (row, head) of q, times the softmax scale; qp 16-byte aligned (global memory or LDS)
__device__ __forceinline__ void load_q_scaled(float (&qr)[D], const float* qp_, float scale) {
    const f4* qp = reinterpret_cast<const f4*>(qp_);
#pragma unroll
    for (int c = 0; c < D / 4; ++c) {
        const f4 t = qp[c];
        qr[4 * c] = t.x * scale; qr[4 * c + 1] = t.y * scale; qr[4 * c + 2] = t.z * scale; qr[4 * c + 3] = t.w * scale;
    }
}

// One query row of one head, on the LPR adjacent lanes that own it (all of them active): lane `part` walks keys part, part + LPR, ...
// with its own online softmax, the partial (m, l, acc) are merged across the lanes, and out = acc / l (zeros when no key is
// valid).  qr: the scaled query.  Ks / Vs: the head's keys / values in LDS, row pitch PITCH floats; valid: u8 per key in LDS.
// Dropout of the attention weights: explicit keep bytes kp[kk] of this (row, head), else the counter-based bit of element
// rbase + kk of batch entry `item` (rbase = (h * Lq + row) * Lk).  Returns the log-sum-exp of the row when WANT_LSE.
template <int PITCH, bool WANT_LSE>
__device__ __forceinline__ float attn_row_head(const float (&qr)[D], const float* Ks, const float* Vs, const unsigned char* valid, int Lk,
                                               int part, const unsigned char* kp, const DropRng& rng, uint64_t seed, uint32_t item,
                                               uint64_t rbase, float keep_scale, float (&out)[D])
{
    float m = -INFINITY, l = 0.f, acc[D];
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = 0.f;
    for (int kk = part; kk < Lk; kk += LPR) {
        if (!valid[kk]) continue;
        const float s = dot16(qr, Ks + kk * PITCH);
        const float mn = fmaxf(m, s);
        const float c = expf(m - mn), e = expf(s - mn);
        l = l * c + e;
        const bool kept = kp ? kp[kk] != 0 : (!rng.thresh || phnet_rng_keep(seed, phnet_rng_index_b(rng, item, rbase + kk), rng.thresh));
        const float ed = kept ? e * keep_scale : 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) acc[d] = acc[d] * c + ed * Vs[kk * PITCH + d];
        m = mn;
    }
    // merge the LPR partial (m, l, acc) of the row
    const float mt = quad_max(m);
    const float c = (m == -INFINITY) ? 0.f : expf(m - mt);
    l = quad_sum(l * c);
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = quad_sum(acc[d] * c);
    const float inv = l > 0.f ? 1.0f / l : 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) out[d] = acc[d] * inv;
    return WANT_LSE ? mt + logf(l) : 0.f;
}

}  // namespace attn_dev
