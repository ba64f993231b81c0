// The AdamW element update, shared by adamw_kernel (elementwise.hip) and adamw_guarded_kernel (optim_guard.hip): one function, so
// that the guarded step on g equals the plain step on fl32(g * mult) by construction (include/phnet_hip.h, "guarded step" rule 8).
#pragma once
#include "common.h"

typedef float adamw_f32x4 __attribute__((ext_vector_type(4)));

// decoupled weight decay on elements [0, n_decay); same update order as torch's single-tensor AdamW:
//   p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= (lr / (1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// Vector i (elements 4i .. 4i+3) of the flat arrays.  SCALED: the gradient the update sees is fl32(g * mult), one rounded f32 multiply
// (__fmul_rn; its result only ever feeds further multiplies, so no mul+add contraction can reach through it).
template <bool SCALED>
__device__ __forceinline__ void adamw_update4(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, long i, long n_decay, const long long* __restrict__ step,
                                              float lr, const float* __restrict__ lr_dev, float b1, float b2, float eps, float wd,
                                              float mult)
{
    if (lr_dev) lr = lr_dev[0];                      // learning rate from device memory: a replayed hipGraph follows the schedule
    const float t = (float)step[0];
    const float c1 = 1.0f - powf(b1, t), c2s = sqrtf(1.0f - powf(b2, t));
    const float step_size = lr / c1;
    adamw_f32x4 pp = reinterpret_cast<adamw_f32x4*>(p)[i], mm = reinterpret_cast<adamw_f32x4*>(m)[i],
                vv = reinterpret_cast<adamw_f32x4*>(v)[i];
    adamw_f32x4 gg = reinterpret_cast<const adamw_f32x4*>(g)[i];
    if (SCALED) {
#pragma unroll
        for (int e = 0; e < 4; ++e) gg[e] = __fmul_rn(gg[e], mult);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float pe = pp[e];
        if (i * 4 + e < n_decay) pe *= 1.0f - lr * wd;
        const float me = b1 * mm[e] + (1.0f - b1) * gg[e];
        const float ve = b2 * vv[e] + (1.0f - b2) * gg[e] * gg[e];
        pe -= step_size * (me / (sqrtf(ve) / c2s + eps));
        pp[e] = pe; mm[e] = me; vv[e] = ve;
    }
    reinterpret_cast<adamw_f32x4*>(p)[i] = pp; reinterpret_cast<adamw_f32x4*>(m)[i] = mm; reinterpret_cast<adamw_f32x4*>(v)[i] = vv;
}
