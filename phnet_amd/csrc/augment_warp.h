// The warp launch of the training augmentation (rules 1 - 6 of include/phnet_hip.h; csrc/augment.hip describes it) as a template, so that
// csrc/augment.hip instantiates the two layouts of phnet_augment_u8 and csrc/augment_stencil.hip the two of phnet_augment_stencil_u8,
// which differ by ONE wave-uniform switch per frame: where a tap comes from.
#pragma once
#include "augment_rules.h"

#pragma clang fp contract(off)

using namespace phnet_aug;

namespace {

constexpr int NT = 256;

// STENCIL: the warp launch of phnet_augment_stencil_u8 with a stencil table - a frame that has a neighbourhood op (rule 7) takes its
// taps from `staged`, where the staging launch left rules 4, 5 and 7 of that frame; every other frame runs the code of STENCIL = false
template <bool NHWC4, bool STENCIL>
__global__ __launch_bounds__(NT) void augment_kernel(
    const uint8_t* __restrict__ src, float* __restrict__ dst, uint8_t* __restrict__ dst_u8, const int32_t* __restrict__ flip2,
    const double* __restrict__ inv, const int32_t* __restrict__ table, const int32_t* __restrict__ stencil,
    const uint8_t* __restrict__ staged, int T, unsigned bpf, int H, int W, float m0, float m1, float m2, float s0, float s1, float s2)
{
#pragma clang fp contract(off)
    const unsigned t = blockIdx.x / bpf;
    const int per = H * W;
    const int rem = (int)((blockIdx.x - t * bpf) * NT + threadIdx.x);
    if (t >= (unsigned)T || rem >= per) return;                     // the grid is T * bpf workgroups: t < T by construction, kept as a guard
    const long i = (long)t * per + rem;
    const int y = rem / W, x = rem - y * W;

    const FrameAug p = load_frame_aug(flip2, table, t);
    bool from_staged = false;                                       // wave-uniform: one frame per workgroup
    if (STENCIL) {
        const int32_t* srow = stencil + (size_t)t * kStencilCols;
        from_staged = stencil_edge(srow) || stencil_kind(srow) != kBlurNone;
    }

    const double* a = inv + (size_t)t * 6;
    const double u = (a[0] * (double)x + a[1] * (double)y) + a[2];
    const double v = (a[3] * (double)x + a[4] * (double)y) + a[5];
    int acc[3] = {0, 0, 0};
    if (u > -2.0 && u < (double)W + 1.0 && v > -2.0 && v < (double)H + 1.0) {
        const int U = (int)floor(u * 32.0 + 0.5), Vq = (int)floor(v * 32.0 + 0.5);
        const int x0 = U >> 5, fx = U & 31, y0 = Vq >> 5, fy = Vq & 31;
        const uint8_t* frame = src + (size_t)t * per * 3;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int yt = y0 + j, wy = j ? fy : 32 - fy;
            if (wy == 0 || yt < 0 || yt >= H) continue;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int xt = x0 + k, w = (k ? fx : 32 - fx) * wy;
                if (w == 0 || xt < 0 || xt >= W) continue;
                int c[3];
                if (STENCIL && from_staged) {                       // B(xt, yt) of rule 7: flipped, coloured, dropped out and filtered already
                    const uint8_t* px = staged + (size_t)t * per * 3 + ((unsigned)(yt * W + xt)) * 3u;
                    c[0] = px[0]; c[1] = px[1]; c[2] = px[2];
                } else {
                    const uint8_t* px = frame + ((unsigned)(yt * W + (p.flip2 ? W - 1 - xt : xt))) * 3u;
                    c[0] = px[0]; c[1] = px[1]; c[2] = px[2];
                    colour(c, p);
                    dropout(c, p, t, xt, yt, H, W);
                }
                acc[0] += w * c[0]; acc[1] += w * c[1]; acc[2] += w * c[2];
            }
        }
    }
    float f[3];
    uint8_t q8[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int q = (acc[c] + 512) >> 10;                         // <= 255: the weights sum to 1024
        q8[c] = (uint8_t)q;
        f[c] = (float)q / 255.0f;
    }
    f[0] = (f[0] - m0) / s0; f[1] = (f[1] - m1) / s1; f[2] = (f[2] - m2) / s2;
    if (dst_u8) { uint8_t* o = dst_u8 + (size_t)i * 3; o[0] = q8[0]; o[1] = q8[1]; o[2] = q8[2]; }
    if (NHWC4) {
        reinterpret_cast<float4*>(dst)[i] = make_float4(f[0], f[1], f[2], 0.f);
    } else {
        float* o = dst + (size_t)t * 3 * per + rem;
        o[0] = f[0]; o[per] = f[1]; o[2 * (size_t)per] = f[2];
    }
}

// the argument checks of both entries and the warp launch.  STENCIL: stencil and staged are not null, and the staging launch
// (`stage`, csrc/augment_stencil.hip) goes first; else both are null: the launch of phnet_augment_u8
template <bool STENCIL>
int augment_launch(const uint8_t* frames, float* out, uint8_t* out_u8, const int32_t* flip2, const double* inv, const int32_t* table,
                   const int32_t* stencil, uint8_t* staged, int32_t T, int32_t H, int32_t W, int32_t layout, const float* mean3_host,
                   const float* std3_host, void* stream,
                   void (*stage)(const uint8_t*, uint8_t*, const int32_t*, const int32_t*, const int32_t*, int, int, int, hipStream_t) = nullptr)
{
    if (T < 0 || H < 1 || W < 1 || H > kMaxSide || W > kMaxSide || (layout != 0 && layout != 1)) return PHNET_ERR_ARG;
    const int64_t per = (int64_t)H * W, bpf = ceil_div64(per, NT);
    if (per * 4 >= INT32_MAX || (int64_t)T * bpf >= INT32_MAX) return PHNET_ERR_ARG;        // byte offsets inside a frame are 32-bit
    if (STENCIL && (int64_t)T * augment_stage_tiles(H, W) >= INT32_MAX) return PHNET_ERR_ARG;
    if (T == 0) return PHNET_OK;
    if (!frames || !out || !flip2 || !inv || !table || !mean3_host || !std3_host || (STENCIL && !staged)) return PHNET_ERR_ARG;
    if (std3_host[0] == 0.f || std3_host[1] == 0.f || std3_host[2] == 0.f) return PHNET_ERR_ARG;
    const dim3 grid((unsigned)(T * bpf));                          // bpf workgroups per frame: a workgroup never straddles two frames
    if (STENCIL) stage(frames, staged, flip2, table, stencil, (int)T, (int)H, (int)W, (hipStream_t)stream);
    const float m0 = mean3_host[0], m1 = mean3_host[1], m2 = mean3_host[2], s0 = std3_host[0], s1 = std3_host[1], s2 = std3_host[2];
#define PHNET_AUGMENT_LAUNCH(NHWC4, STENCIL)                                                                                           \
    hipLaunchKernelGGL((augment_kernel<NHWC4, STENCIL>), grid, dim3(NT), 0, (hipStream_t)stream, frames, out, out_u8, flip2, inv, table, \
                       stencil, (const uint8_t*)staged, (int)T, (unsigned)bpf, (int)H, (int)W, m0, m1, m2, s0, s1, s2)
    if (layout == 1) PHNET_AUGMENT_LAUNCH(true, STENCIL); else PHNET_AUGMENT_LAUNCH(false, STENCIL);
#undef PHNET_AUGMENT_LAUNCH
    return phnet_launch_status();
}

}  // namespace
