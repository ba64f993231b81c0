// The neighbourhood ops of the training augmentation (rule 7 of include/phnet_hip.h; DESIGN.md "Training augmentation"): EdgeDetect /
// DirectedEdgeDetect and MotionBlur / MedianBlur / GaussianBlur of the reference's 'complex' recipe (libs/dataset/openlane/
// transforms.py:220-238).  They cannot run on the four taps of the warp (csrc/augment.hip): a 5 x 5 median between the dropout and the
// warp would multiply the work of every tap by 25.  So a frame that has such an op takes ONE staging pass, this launch, which writes
//     B = blur(dropout(edge(colour(flip(source)))))                                                       (rules 4, 7 edge, 5, 7 blur)
// as an 8-bit image into `staged`, and the warp launch then reads its taps from there.  tests/stencil_cases.py restates it in numpy.
//
// One 256-thread workgroup per 64 x 16 tile of a frame.  It reads the frame's stencil row as wave-uniform loads and returns at once when
// the frame has neither op, so the launch is in the graph whatever the table holds at replay.  Otherwise, with R the blur radius (0 - 4):
//   1. C (rule 4) on the tile + R + (edge ? 1 : 0) into LDS, one packed RGBX dword per pixel;
//   2. E (the 3 x 3 edge filter, Q12) and D (rule 5) on the tile + R into a second LDS tile;
//   3. B on the tile: a k x k Q12 convolution, a k x k median (a min / max network in registers, per channel), or the separable Q8
//      Gaussian with its horizontal sums in LDS as 32-bit values; written to `staged`.
// Both LDS tiles hold IN-IMAGE pixels only, [max(0, lo - halo), min(n - 1, hi + halo)] each way: a tap is mapped into the image first
// (reflect-101, or replicate for the median) and then looked up, so an image smaller than the radius, where a reflection wraps more than
// once, needs nothing special.  Every mapped tap of a tile lies in that range: a reflected index is at most halo inside the border.
// Rows of consecutive dwords: 64 lanes on 64 consecutive pixels are conflict-free for ds_read_b32.  LDS 33 040 B per workgroup.
// Integer arithmetic throughout; all sums stay inside int32 under the clamps of the table (|e| <= 2^16: 9 * 2^16 * 255 < 2^28;
// m <= 2^16: 25 * 2^16 * 255 < 2^29; g <= 2^8: 81 * 2^16 * 255 < 2^31 - 2^15).
#include "augment_warp.h"

namespace {

constexpr int TW = kStageTileW, TH = kStageTileH;                   // the tile: a row of it is one wave
constexpr int DW = TW + 2 * kMaxRadius, DH = TH + 2 * kMaxRadius;   // the D tile at most
constexpr int CW = DW + 2, CH = DH + 2;                             // the C tile at most

__device__ __forceinline__ uint32_t pack(const int (&c)[3]) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }
__device__ __forceinline__ int chan(uint32_t q, int k) { return (int)((q >> (8 * k)) & 255u); }

// the in-image pixels a workgroup holds in LDS and the outputs it owns
struct Tile {
    int x0, y0, ox1, oy1;                     // outputs [x0, ox1] x [y0, oy1]
    int dx0, dy0, dw, dh;                     // D: [dx0, dx0 + dw) x [dy0, dy0 + dh)
};

// the median of N = k * k values, N = 9 or 25: keep N / 2 + 2 candidates, drop their minimum and their maximum (neither can be the
// median), take the next value in, until three are left.  Fully unrolled: every index is a constant, the values stay in registers
template <int N>
__device__ __forceinline__ int median_of(const int (&v)[N])
{
    constexpr int S0 = N / 2 + 2;
    int a[S0];
#pragma unroll
    for (int i = 0; i < S0; ++i) a[i] = v[i];
#pragma unroll
    for (int s = S0; s > 3; --s) {
#pragma unroll
        for (int i = 0; i < s / 2; ++i) { const int lo = min(a[i], a[s - 1 - i]), hi = max(a[i], a[s - 1 - i]); a[i] = lo; a[s - 1 - i] = hi; }
#pragma unroll
        for (int i = 1; i <= (s - 1) / 2; ++i) { const int lo = min(a[0], a[i]), hi = max(a[0], a[i]); a[0] = lo; a[i] = hi; }
#pragma unroll
        for (int i = s / 2; i < s - 1; ++i) { const int lo = min(a[i], a[s - 1]), hi = max(a[i], a[s - 1]); a[i] = lo; a[s - 1] = hi; }
        a[0] = v[N - (s - 3)];                                      // the minimum leaves, the next value comes; a[s - 1] is dropped
    }
    return max(min(a[0], a[1]), min(max(a[0], a[1]), a[2]));
}

template <int K>
__device__ __forceinline__ void blur_motion(const uint32_t* sD, const Tile& g, const int32_t* __restrict__ srow, int x, int y, int H, int W,
                                            int (&out)[3])
{
    constexpr int R = K / 2;
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int base = (reflect101(y + j - R, H) - g.dy0) * g.dw - g.dx0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const int w = clampi(srow[kBlurW0 + j * K + i], 0, 65536);
            const uint32_t q = sD[base + reflect101(x + i - R, W)];
            acc[0] += w * chan(q, 0); acc[1] += w * chan(q, 1); acc[2] += w * chan(q, 2);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = clampi((acc[c] + 2048) >> 12, 0, 255);
}

template <int K>
__device__ __forceinline__ void blur_median(const uint32_t* sD, const Tile& g, int x, int y, int H, int W, int (&out)[3])
{
    constexpr int R = K / 2;
    uint32_t q[K * K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int base = (clampi(y + j - R, 0, H - 1) - g.dy0) * g.dw - g.dx0;
#pragma unroll
        for (int i = 0; i < K; ++i) q[j * K + i] = sD[base + clampi(x + i - R, 0, W - 1)];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int v[K * K];
#pragma unroll
        for (int n = 0; n < K * K; ++n) v[n] = chan(q[n], c);
        out[c] = median_of<K * K>(v);
    }
}

// the Gaussian of radius R on the tile: horizontal sums of the D rows into sH, then the vertical pass.  Called by the whole workgroup
template <int R>
__device__ __forceinline__ void blur_gauss(const uint32_t* sD, int (*sH)[TW * DH], const Tile& g, const int32_t* __restrict__ srow,
                                           uint8_t* __restrict__ dst, int H, int W)
{
    constexpr int K = 2 * R + 1;
    int w[K];
#pragma unroll
    for (int i = 0; i < K; ++i) w[i] = clampi(srow[kBlurW0 + i], 0, 256);
    for (int idx = threadIdx.x; idx < TW * g.dh; idx += NT) {
        const int yy = idx / TW, xx = idx - yy * TW, x = g.x0 + xx;
        if (x > g.ox1) continue;
        const int base = yy * g.dw - g.dx0;
        int acc[3] = {0, 0, 0};
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const uint32_t q = sD[base + reflect101(x + i - R, W)];
            acc[0] += w[i] * chan(q, 0); acc[1] += w[i] * chan(q, 1); acc[2] += w[i] * chan(q, 2);
        }
        sH[0][idx] = acc[0]; sH[1][idx] = acc[1]; sH[2][idx] = acc[2];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < TW * TH; idx += NT) {
        const int yy = idx / TW, xx = idx - yy * TW, x = g.x0 + xx, y = g.y0 + yy;
        if (x > g.ox1 || y > g.oy1) continue;
        int acc[3] = {0, 0, 0};
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int at = (reflect101(y + j - R, H) - g.dy0) * TW + xx;
            acc[0] += w[j] * sH[0][at]; acc[1] += w[j] * sH[1][at]; acc[2] += w[j] * sH[2][at];
        }
        uint8_t* o = dst + ((unsigned)(y * W + x)) * 3u;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (uint8_t)clampi((acc[c] + 32768) >> 16, 0, 255);
    }
}

__global__ __launch_bounds__(NT) void augment_stage_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ staged, const int32_t* __restrict__ flip2, const int32_t* __restrict__ table,
    const int32_t* __restrict__ stencil, int T, unsigned tiles_x, unsigned tiles, int H, int W)
{
    __shared__ uint32_t sC[CW * CH];
    __shared__ uint32_t sD[DW * DH];
    __shared__ int sH[3][TW * DH];

    const unsigned t = blockIdx.x / tiles;
    if (t >= (unsigned)T) return;                                   // the grid is T * tiles workgroups: kept as a guard
    const int32_t* srow = stencil + (size_t)t * kStencilCols;
    const bool edge = stencil_edge(srow);
    const int kind = stencil_kind(srow);
    if (!edge && kind == kBlurNone) return;                         // the warp launch runs rules 4 and 5 itself on this frame
    const int R = stencil_radius(srow, kind), eh = edge ? 1 : 0;
    const FrameAug p = load_frame_aug(flip2, table, t);

    const unsigned tile = blockIdx.x - t * tiles, tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
    Tile g;
    g.x0 = (int)txi * TW; g.y0 = (int)tyi * TH;
    g.ox1 = min(g.x0 + TW - 1, W - 1); g.oy1 = min(g.y0 + TH - 1, H - 1);
    g.dx0 = max(0, g.x0 - R); g.dy0 = max(0, g.y0 - R);
    g.dw = min(W - 1, g.ox1 + R) - g.dx0 + 1; g.dh = min(H - 1, g.oy1 + R) - g.dy0 + 1;
    const int cx0 = max(0, g.dx0 - eh), cy0 = max(0, g.dy0 - eh);
    const int cw = min(W - 1, g.dx0 + g.dw - 1 + eh) - cx0 + 1, ch = min(H - 1, g.dy0 + g.dh - 1 + eh) - cy0 + 1;
    const int per = H * W;
    const uint8_t* frame = src + (size_t)t * per * 3;

    // 1. C: flip and rule 4
    for (int idx = threadIdx.x; idx < cw * ch; idx += NT) {
        const int yy = idx / cw, x = cx0 + (idx - yy * cw), y = cy0 + yy;
        const uint8_t* px = frame + ((unsigned)(y * W + (p.flip2 ? W - 1 - x : x))) * 3u;
        int c[3] = {px[0], px[1], px[2]};
        colour(c, p);
        sC[idx] = pack(c);
    }
    __syncthreads();

    // 2. E, then D: rule 5 at the pixel's own coordinates
    int e[9];
#pragma unroll
    for (int n = 0; n < 9; ++n) e[n] = clampi(srow[kEdge0 + n], -65536, 65536);
    for (int idx = threadIdx.x; idx < g.dw * g.dh; idx += NT) {
        const int yy = idx / g.dw, x = g.dx0 + (idx - yy * g.dw), y = g.dy0 + yy;
        int c[3];
        if (edge) {
            int acc[3] = {0, 0, 0};
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int base = (reflect101(y + j - 1, H) - cy0) * cw - cx0;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const uint32_t q = sC[base + reflect101(x + i - 1, W)];
                    acc[0] += e[j * 3 + i] * chan(q, 0); acc[1] += e[j * 3 + i] * chan(q, 1); acc[2] += e[j * 3 + i] * chan(q, 2);
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = clampi((acc[k] + 2048) >> 12, 0, 255);
        } else {
            const uint32_t q = sC[(y - cy0) * cw + (x - cx0)];
            c[0] = chan(q, 0); c[1] = chan(q, 1); c[2] = chan(q, 2);
        }
        dropout(c, p, t, x, y, H, W);
        sD[idx] = pack(c);
    }
    __syncthreads();

    // 3. B
    uint8_t* dst = staged + (size_t)t * per * 3;
    if (kind == kBlurGauss) {                                       // wave-uniform, as R is
        if (R == 1) blur_gauss<1>(sD, sH, g, srow, dst, H, W);
        else if (R == 2) blur_gauss<2>(sD, sH, g, srow, dst, H, W);
        else if (R == 3) blur_gauss<3>(sD, sH, g, srow, dst, H, W);
        else blur_gauss<4>(sD, sH, g, srow, dst, H, W);
        return;
    }
    for (int idx = threadIdx.x; idx < TW * TH; idx += NT) {
        const int yy = idx / TW, xx = idx - yy * TW, x = g.x0 + xx, y = g.y0 + yy;
        if (x > g.ox1 || y > g.oy1) continue;
        int c[3];
        if (kind == kBlurMotion) {
            if (R == 1) blur_motion<3>(sD, g, srow, x, y, H, W, c); else blur_motion<5>(sD, g, srow, x, y, H, W, c);
        } else if (kind == kBlurMedian) {
            if (R == 1) blur_median<3>(sD, g, x, y, H, W, c); else blur_median<5>(sD, g, x, y, H, W, c);
        } else {
            const uint32_t q = sD[(y - g.dy0) * g.dw + (x - g.dx0)];
            c[0] = chan(q, 0); c[1] = chan(q, 1); c[2] = chan(q, 2);
        }
        uint8_t* o = dst + ((unsigned)(y * W + x)) * 3u;
        o[0] = (uint8_t)c[0]; o[1] = (uint8_t)c[1]; o[2] = (uint8_t)c[2];
    }
}

void launch_augment_stage(const uint8_t* frames, uint8_t* staged, const int32_t* flip2, const int32_t* table, const int32_t* stencil,
                          int T, int H, int W, hipStream_t stream)
{
    const unsigned tiles_x = (unsigned)ceil_div64(W, TW), tiles = (unsigned)augment_stage_tiles(H, W);     // T * tiles < 2^31: checked
    hipLaunchKernelGGL(augment_stage_kernel, dim3((unsigned)T * tiles), dim3(NT), 0, stream, frames, staged, flip2, table, stencil, T,
                       tiles_x, tiles, H, W);
}

}  // namespace

PHNET_API int phnet_augment_u8(const uint8_t* frames, float* out, uint8_t* out_u8, const int32_t* flip2, const double* inv,
                               const int32_t* table, int32_t T, int32_t H, int32_t W, int32_t layout, const float* mean3_host,
                               const float* std3_host, void* stream);                  // csrc/augment.hip

// phnet_augment_u8 with the neighbourhood ops of rule 7: stencil i32 [T][40] on the device (nullptr: phnet_augment_u8 itself), staged u8
// [T][H][W][3] caller-owned scratch on the device.  Two launches: the staging launch above writes B of the frames that have such an op into
// `staged`, then the warp launch (csrc/augment_warp.h) reads its taps there for those frames.
PHNET_API int phnet_augment_stencil_u8(const uint8_t* frames, float* out, uint8_t* out_u8, const int32_t* flip2, const double* inv,
                                       const int32_t* table, const int32_t* stencil, uint8_t* staged, int32_t T, int32_t H, int32_t W,
                                       int32_t layout, const float* mean3_host, const float* std3_host, void* stream)
{
    if (!stencil) return phnet_augment_u8(frames, out, out_u8, flip2, inv, table, T, H, W, layout, mean3_host, std3_host, stream);
    return augment_launch<true>(frames, out, out_u8, flip2, inv, table, stencil, staged, T, H, W, layout, mean3_host, std3_host, stream,
                                launch_augment_stage);
}
