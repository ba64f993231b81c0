// Training augmentation of a clip on the GPU: the resized 8-bit RGB frames (the out_u8 of csrc/preprocess.hip) -> the warped, recoloured,
// dropped-out and normalised float clip, one launch, no intermediate image (DESIGN.md "Training augmentation").  The image half of the
// point-wise part of the reference's imgaug pipeline (libs/dataset/openlane/transforms.py:190-249: HorizontalFlip, ChannelShuffle,
// MultiplyAndAddToBrightness, AddToHueAndSaturation, Dropout / CoarseDropout, Affine); the label half is rule 0b of csrc/lane_targets.hip.
// Every parameter comes from a per-frame table in device memory, so a captured launch picks up new parameters at every replay.
//
// Rules, for output pixel (x, y) of frame t (include/phnet_hip.h states them for callers; tests/augment_cases.py restates them in numpy):
//   1. u = (a00 x + a01 y) + a02, v = (a10 x + a11 y) + a12 in double, not contracted; a = inv[t], the output -> source matrix.
//   2. not (-2 < u < W + 1 and -2 < v < H + 1) (NaN included): the pixel is the fill colour.  Else U = floor(u * 32 + 0.5), x0 = U >> 5,
//      fx = U & 31, the same for v: taps (x0 + i, y0 + j), i, j in {0, 1}, weights (32 - fx, fx) x (32 - fy, fy), sum 1024.
//   3. a tap outside [0, W) x [0, H) is 0, 0, 0; an inside tap (xt, yt) is the source pixel (flip2 ? W - 1 - xt : xt, yt) after rules 4, 5.
//   4. colour: permutation; brightness on V = max(R, G, B); hue / saturation in a 24576-step integer HSV.  Each is skipped when neutral.
//   5. dropout: per pixel or per cell of a gh x gw grid, phnet_rng_keep of common.h on the element's index.
//   6. (sum of weight * tap + 512) >> 10 per channel; then q / 255, (v - mean) / std in f32: the epilogue of csrc/preprocess.hip.
//
// One thread per output pixel, 256-thread workgroups that stay inside one frame, so the frame's 22 table words are wave-uniform loads and
// every branch on an op being switched on is wave-uniform.  At most 4 taps x 3 byte loads per pixel (1 tap x 3 with an integer shift),
// 12 - 16 bytes written.  Integer arithmetic from the taps to the 8-bit result; the only floating point is rule 1 (f64) and the epilogue.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int kMaxSide = 32768;               // H, W: 32 * (W + 3) and yt * gh stay far inside int32
constexpr int kHueSteps = 24576;              // one turn of hue: 6 sextants of 4096 steps

// columns of the i32 table [T][16]
enum { kPerm0 = 0, kPerm1, kPerm2, kMulQ, kAdd, kHueSat, kDropMode, kPerChannel, kThresh, kGridH, kGridW, kSeedLo, kSeedHi, kCols = 16 };

struct FrameAug {
    int flip2, perm[3], mq, add, hs, mode, per_channel, gh, gw;
    uint32_t thresh;
    uint64_t seed;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int floor_div(int a, int b) { return a >= 0 ? a / b : -((b - 1 - a) / b); }      // b > 0

// rule 4 on one tap
__device__ __forceinline__ void colour(int (&c)[3], const FrameAug& p)
{
    if (p.perm[0] != 0 || p.perm[1] != 1 || p.perm[2] != 2) {
        const int s[3] = {c[0], c[1], c[2]};
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = p.perm[k] == 0 ? s[0] : (p.perm[k] == 1 ? s[1] : s[2]);
    }
    if (p.mq != 256 || p.add != 0) {
        const int V = max(c[0], max(c[1], c[2]));
        const int V2 = clampi(((V * p.mq + 128) >> 8) + p.add, 0, 255);
        if (V == 0) {
            c[0] = c[1] = c[2] = V2;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = (2 * c[k] * V2 + V) / (2 * V);
        }
    }
    if (p.hs != 0) {
        const int R = c[0], G = c[1], B = c[2];
        const int V = max(R, max(G, B)), C = V - min(R, min(G, B));
        const int S = V == 0 ? 0 : (510 * C + V) / (2 * V);
        int h = 0;
        if (C != 0) {
            int base, d;
            if (V == R) { base = 0; d = G - B; } else if (V == G) { base = 8192; d = B - R; } else { base = 16384; d = R - G; }
            h = (base + ((d + C) * 8192 + C) / (2 * C) - 4096 + kHueSteps) % kHueSteps;
        }
        const int S2 = clampi(S + p.hs, 0, 255);
        const int C2 = (2 * V * S2 + 255) / 510;
        const int dh = floor_div(p.hs * (2 * kHueSteps) + 255, 510);
        const int h2 = ((h + dh) % kHueSteps + kHueSteps) % kHueSteps;
        const int i = h2 >> 12, f = h2 & 4095;
        const int lo = V - C2, q = V - ((C2 * f + 2048) >> 12), t = V - ((C2 * (4096 - f) + 2048) >> 12);
        c[0] = (i == 0 || i == 5) ? V : (i == 1 ? q : (i == 4 ? t : lo));
        c[1] = (i == 1 || i == 2) ? V : (i == 3 ? q : (i == 0 ? t : lo));
        c[2] = (i == 3 || i == 4) ? V : (i == 5 ? q : (i == 2 ? t : lo));
    }
}

// rule 5 on one tap at (xt, yt) of frame t
__device__ __forceinline__ void dropout(int (&c)[3], const FrameAug& p, unsigned t, int xt, int yt, int H, int W)
{
    if (p.mode != 1 && p.mode != 2) return;
    uint64_t e;
    if (p.mode == 1) e = ((uint64_t)t * (uint64_t)H + (uint64_t)yt) * (uint64_t)W + (uint64_t)xt;
    else e = ((uint64_t)t * (uint64_t)p.gh + (uint64_t)((yt * p.gh) / H)) * (uint64_t)p.gw + (uint64_t)((xt * p.gw) / W);
    if (p.per_channel) {
#pragma unroll
        for (int k = 0; k < 3; ++k) if (!phnet_rng_keep(p.seed, e * 3 + k, p.thresh)) c[k] = 0;
    } else if (!phnet_rng_keep(p.seed, e, p.thresh)) {
        c[0] = c[1] = c[2] = 0;
    }
}

template <bool NHWC4>
__global__ __launch_bounds__(NT) void augment_kernel(
    const uint8_t* __restrict__ src, float* __restrict__ dst, uint8_t* __restrict__ dst_u8, const int32_t* __restrict__ flip2,
    const double* __restrict__ inv, const int32_t* __restrict__ table, int T, unsigned bpf, int H, int W,
    float m0, float m1, float m2, float s0, float s1, float s2)
{
#pragma clang fp contract(off)
    const unsigned t = blockIdx.x / bpf;
    const int per = H * W;
    const int rem = (int)((blockIdx.x - t * bpf) * NT + threadIdx.x);
    if (t >= (unsigned)T || rem >= per) return;                     // the grid is T * bpf workgroups: t < T by construction, kept as a guard
    const long i = (long)t * per + rem;
    const int y = rem / W, x = rem - y * W;

    // the frame's parameters, clamped so that no table can index out of bounds or overflow
    const int32_t* row = table + (size_t)t * kCols;
    FrameAug p;
    p.flip2 = flip2[t] != 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) p.perm[k] = clampi(row[kPerm0 + k], 0, 2);
    p.mq = clampi(row[kMulQ], 0, 65536);
    p.add = clampi(row[kAdd], -255, 255);
    p.hs = clampi(row[kHueSat], -255, 255);
    p.mode = row[kDropMode];
    p.per_channel = row[kPerChannel] != 0;
    p.thresh = (uint32_t)row[kThresh];
    p.gh = clampi(row[kGridH], 1, kMaxSide);
    p.gw = clampi(row[kGridW], 1, kMaxSide);
    p.seed = ((uint64_t)(uint32_t)row[kSeedHi] << 32) | (uint64_t)(uint32_t)row[kSeedLo];

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
                const uint8_t* px = frame + ((unsigned)(yt * W + (p.flip2 ? W - 1 - xt : xt))) * 3u;
                int c[3] = {px[0], px[1], px[2]};
                colour(c, p);
                dropout(c, p, t, xt, yt, H, W);
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

}  // namespace

// frames u8 [T][H][W][3] (device; the out_u8 of phnet_preprocess_u8 / _yuv), out f32 NCHW [T][3][H][W] (layout 0) or NHWC4 [T][H][W][4]
// (layout 1), out_u8 optional [T][H][W][3]; flip2 i32 [T], inv f64 [T][6], table i32 [T][16] on the device; mean3 / std3 HOST pointers.
PHNET_API int phnet_augment_u8(const uint8_t* frames, float* out, uint8_t* out_u8, const int32_t* flip2, const double* inv,
                               const int32_t* table, int32_t T, int32_t H, int32_t W, int32_t layout, const float* mean3_host,
                               const float* std3_host, void* stream)
{
    if (T < 0 || H < 1 || W < 1 || H > kMaxSide || W > kMaxSide || (layout != 0 && layout != 1)) return PHNET_ERR_ARG;
    const int64_t per = (int64_t)H * W, bpf = ceil_div64(per, NT);
    if (per * 4 >= INT32_MAX || (int64_t)T * bpf >= INT32_MAX) return PHNET_ERR_ARG;        // byte offsets inside a frame are 32-bit
    if (T == 0) return PHNET_OK;
    if (!frames || !out || !flip2 || !inv || !table || !mean3_host || !std3_host) return PHNET_ERR_ARG;
    if (std3_host[0] == 0.f || std3_host[1] == 0.f || std3_host[2] == 0.f) return PHNET_ERR_ARG;
    const dim3 grid((unsigned)(T * bpf));                          // bpf workgroups per frame: a workgroup never straddles two frames
    const float m0 = mean3_host[0], m1 = mean3_host[1], m2 = mean3_host[2], s0 = std3_host[0], s1 = std3_host[1], s2 = std3_host[2];
    if (layout == 1)
        hipLaunchKernelGGL(augment_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, frames, out, out_u8, flip2, inv, table, (int)T,
                           (unsigned)bpf, (int)H, (int)W, m0, m1, m2, s0, s1, s2);
    else
        hipLaunchKernelGGL(augment_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, frames, out, out_u8, flip2, inv, table, (int)T,
                           (unsigned)bpf, (int)H, (int)W, m0, m1, m2, s0, s1, s2);
    return phnet_launch_status();
}
