// The pieces of the training augmentation that its two translation units share (DESIGN.md "Training augmentation"): the per-frame
// parameter loader with its clamps, rule 4 (colour) and rule 5 (dropout) on one pixel, reflect-101, and the columns and the clamps of the
// stencil table.  csrc/augment_warp.h (the warp launch) and csrc/augment_stencil.hip (the staging launch of the neighbourhood
// ops) include it; include/phnet_hip.h states the rules for callers.
#pragma once
#include "common.h"

namespace phnet_aug {

constexpr int kMaxSide = 32768;               // H, W: 32 * (W + 3) and yt * gh stay far inside int32
constexpr int kHueSteps = 24576;              // one turn of hue: 6 sextants of 4096 steps

// columns of the i32 table [T][16]
enum { kPerm0 = 0, kPerm1, kPerm2, kMulQ, kAdd, kHueSat, kDropMode, kPerChannel, kThresh, kGridH, kGridW, kSeedLo, kSeedHi, kCols = 16 };
// columns of the i32 stencil table [T][40]
enum { kEdgeOn = 0, kEdge0 = 1, kBlurKind = 10, kBlurK = 11, kBlurW0 = 12, kStencilCols = 40 };
enum { kBlurNone = 0, kBlurMotion = 1, kBlurMedian = 2, kBlurGauss = 3 };
constexpr int kMaxRadius = 4;                 // the 9-tap Gaussian

struct FrameAug {
    int flip2, perm[3], mq, add, hs, mode, per_channel, gh, gw;
    uint32_t thresh;
    uint64_t seed;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int floor_div(int a, int b) { return a >= 0 ? a / b : -((b - 1 - a) / b); }      // b > 0

// the frame's parameters, clamped so that no table can index out of bounds or overflow
__device__ __forceinline__ FrameAug load_frame_aug(const int32_t* __restrict__ flip2, const int32_t* __restrict__ table, unsigned t)
{
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
    return p;
}

// rule 4 on one pixel
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

// rule 5 on one pixel at (xt, yt) of frame t
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

// r(i, n) of rule 7: reflect-101, defined for every i.  n in [1, 32768], |i| < 2^30
__device__ __forceinline__ int reflect101(int i, int n)
{
    if ((unsigned)i < (unsigned)n) return i;
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// the clamps of the stencil row (rule 7): what the staging launch does to a frame, and whether the warp launch reads `staged` for it.
// Both kernels decide with these two functions, so they cannot disagree about a frame.
__device__ __forceinline__ int stencil_kind(const int32_t* __restrict__ srow)
{
    const int kind = srow[kBlurKind];
    return kind >= kBlurMotion && kind <= kBlurGauss ? kind : kBlurNone;
}
__device__ __forceinline__ bool stencil_edge(const int32_t* __restrict__ srow) { return srow[kEdgeOn] != 0; }
// k clamped to [3, 5] (motion, median) or [3, 9] (Gaussian) and an even k raised by one -> the radius
__device__ __forceinline__ int stencil_radius(const int32_t* __restrict__ srow, int kind)
{
    if (kind == kBlurNone) return 0;
    return (clampi(srow[kBlurK], 3, kind == kBlurGauss ? 9 : 5) | 1) >> 1;
}

// the tile of one staging workgroup (csrc/augment_stencil.hip; a row of it is one wave) and the workgroups of one frame
constexpr int kStageTileW = 64, kStageTileH = 16;
static inline int64_t augment_stage_tiles(int H, int W) { return ceil_div64(W, kStageTileW) * ceil_div64(H, kStageTileH); }

}  // namespace phnet_aug
