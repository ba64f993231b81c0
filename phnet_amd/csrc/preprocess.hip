// Input pre-processing of a clip on the GPU: decoded uint8 RGB frames -> the float tensor the
// model consumes, one launch per clip.  Replaces, for the image half of the reference's data pipeline,
//   libs/dataset/openlane/datasetOL.py:40-52  (crop the top `crop_size` rows, optional left-right flip)
//   libs/dataset/openlane/transforms.py:150-156 (iaa.Resize -> cv2 INTER_CUBIC on the uint8 image)
//   libs/dataset/openlane/datasetOL.py:63-75, 11-17 (ToTensor /255, Normalize(mean, std), stacking of the frames)
// which the reference runs per frame on CPU data-loader workers; at the inference rates of this implementation (1 500
// frames/s) that is the next bottleneck.
//
// Arithmetic: OpenCV's 8-bit bicubic resize (half-pixel centres, a = -0.75, 11-bit fixed-point taps stored per tap without renormalisation,
// replicated borders, rounding 22-bit shift, saturation) followed by x/255 and (x - mean)/std in f32.  The tap tables are
// built on the host side of the C-ABI once per geometry and passed in (idx [n][4] int32, coef [n][4] int16 per axis).
// HBM-bound: 16 source bytes x 3 channels per output pixel (L2-served re-reads), 12-16 bytes written.
//
// Camera formats (phnet_preprocess_yuv): NV12 and YUYV surfaces enter the same launch; every tap is converted to 8-bit RGB in
// integers first (a 20-bit fixed-point matrix built by the host), so no RGB image is ever written to memory.
#include "common.h"
#include "csc.h"

namespace {

constexpr int NT = 256;

// the epilogue of both kernels: 22-bit rounding shift + saturation of the three bicubic sums, then q/255 and (v - mean)/std in f32
template <bool NHWC4>
__device__ __forceinline__ void store_pixel(const int (&acc)[3], float* __restrict__ dst, uint8_t* __restrict__ dst_u8, long i, int t, int rem,
                                            long per, float m0, float m1, float m2, float s0, float s1, float s2)
{
    float v[3];
    uint8_t u[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int q = (acc[c] + (1 << 21)) >> 22;
        q = q < 0 ? 0 : (q > 255 ? 255 : q);
        u[c] = (uint8_t)q;
        v[c] = (float)q / 255.0f;
    }
    v[0] = (v[0] - m0) / s0; v[1] = (v[1] - m1) / s1; v[2] = (v[2] - m2) / s2;
    if (dst_u8) { uint8_t* o = dst_u8 + (size_t)i * 3; o[0] = u[0]; o[1] = u[1]; o[2] = u[2]; }
    if (NHWC4) {
        reinterpret_cast<float4*>(dst)[i] = make_float4(v[0], v[1], v[2], 0.f);
    } else {
        float* o = dst + (size_t)t * 3 * per + rem;
        o[0] = v[0]; o[per] = v[1]; o[2 * per] = v[2];
    }
}

// one thread per output pixel: 4x4 taps x 3 channels
template <bool NHWC4>
__global__ __launch_bounds__(NT) void preprocess_kernel(
    const uint8_t* __restrict__ src, float* __restrict__ dst, uint8_t* __restrict__ dst_u8,
    const int32_t* __restrict__ xi, const int16_t* __restrict__ xc, const int32_t* __restrict__ yi, const int16_t* __restrict__ yc,
    int T, int H0, int W0, int crop_top, int out_h, int out_w, int flip,
    float m0, float m1, float m2, float s0, float s1, float s2)
{
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    const long per = (long)out_h * out_w;
    if (i >= (long)T * per) return;
    const int t = (int)(i / per);
    const int rem = (int)(i - (long)t * per);
    const int oy = rem / out_w, ox = rem - oy * out_w;
    const uint8_t* frame = src + (size_t)t * H0 * W0 * 3 + (size_t)crop_top * W0 * 3;
    const int Wc = W0;
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint8_t* row = frame + (size_t)yi[oy * 4 + r] * Wc * 3;
        int h[3] = {0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int x = xi[ox * 4 + q];
            if (flip) x = Wc - 1 - x;
            const uint8_t* px = row + (size_t)x * 3;
            const int c = xc[ox * 4 + q];
            h[0] += px[0] * c; h[1] += px[1] * c; h[2] += px[2] * c;
        }
        const int cy = yc[oy * 4 + r];
        acc[0] += h[0] * cy; acc[1] += h[1] * cy; acc[2] += h[2] * cy;
    }
    store_pixel<NHWC4>(acc, dst, dst_u8, i, t, rem, per, m0, m1, m2, s0, s1, s2);
}

// ---- camera formats: the same launch with the colour conversion in front of the taps (no RGB image in memory) ----
// (Csc and csc_channel, the integer conversion of one source pixel: csc.h, shared with lane_draw.hip)

// one thread per output pixel: each of its 4x4 taps is converted to 8-bit RGB first, chroma replicated (never interpolated).
// YUYV = false: NV12, luma rows of `pitch` bytes at the frame's start, interleaved UV rows of `pitch` bytes from chroma_offset on,
// row r >> 1 of them for ABSOLUTE luma row r;  YUYV = true: rows of `pitch` bytes Y0 U Y1 V ...
// A workgroup stays inside one frame (bpf workgroups per frame), so the frame's base is wave-uniform and every load is that base +
// a 32-bit byte offset (a frame spans < 2^31 bytes: checked by the entry).
// The launch is bound by the number of load instructions, not by bytes or arithmetic (with byte loads, 48 per pixel against the RGB
// kernel's 32, it takes 1.26x the RGB launch however cheap the conversion is).  WIDE: where the entry finds base, stride, pitch (and
// chroma offset) aligned, a tap's U,V are ONE 16-bit load (NV12: 32 loads) and a YUYV tap's four bytes ONE 32-bit load (16 loads).
template <bool NHWC4, bool YUYV, bool WIDE>
__global__ __launch_bounds__(NT) void preprocess_yuv_kernel(
    const uint8_t* __restrict__ src, float* __restrict__ dst, uint8_t* __restrict__ dst_u8,
    const int32_t* __restrict__ xi, const int16_t* __restrict__ xc, const int32_t* __restrict__ yi, const int16_t* __restrict__ yc,
    int T, unsigned bpf, int W0, int crop_top, int out_h, int out_w, int flip, long frame_stride, unsigned pitch, unsigned chroma_offset, Csc k,
    float m0, float m1, float m2, float s0, float s1, float s2)
{
    const unsigned t = blockIdx.x / bpf;
    const int per = out_h * out_w;
    const int rem = (int)((blockIdx.x - t * bpf) * NT + threadIdx.x);
    if (t >= (unsigned)T || rem >= per) return;                     // the grid is T * bpf workgroups: t < T by construction, kept as a guard
    const long i = (long)t * per + rem;
    const int oy = rem / out_w, ox = rem - oy * out_w;
    const uint8_t* frame = src + (size_t)t * frame_stride;
    unsigned xs[4];
    int cx[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int x = xi[ox * 4 + q];
        xs[q] = (unsigned)(flip ? W0 - 1 - x : x);
        cx[q] = xc[ox * 4 + q];
    }
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned ar = (unsigned)(crop_top + yi[oy * 4 + r]);      // absolute row: chroma parity follows the uncropped frame
        const unsigned yrow = ar * pitch;
        const unsigned crow = YUYV ? yrow : chroma_offset + (ar >> 1) * pitch;
        int h[3] = {0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned x = xs[q];
            int Y, U, V;
            if (YUYV && WIDE) {                                                       // Y0 U Y1 V, little-endian
                const unsigned w = *reinterpret_cast<const uint32_t*>(frame + (yrow + 4 * (x >> 1)));
                Y = (x & 1) ? (w >> 16) & 0xff : w & 0xff; U = (w >> 8) & 0xff; V = w >> 24;
            } else if (YUYV) {
                Y = frame[yrow + 2 * x]; U = frame[crow + 4 * (x >> 1) + 1]; V = frame[crow + 4 * (x >> 1) + 3];
            } else if (WIDE) {
                const unsigned uv = *reinterpret_cast<const uint16_t*>(frame + (crow + 2 * (x >> 1)));
                Y = frame[yrow + x]; U = uv & 0xff; V = uv >> 8;
            } else {
                Y = frame[yrow + x]; U = frame[crow + 2 * (x >> 1)]; V = frame[crow + 2 * (x >> 1) + 1];
            }
            h[0] += csc_channel(k, 0, Y, U, V) * cx[q];
            h[1] += csc_channel(k, 1, Y, U, V) * cx[q];
            h[2] += csc_channel(k, 2, Y, U, V) * cx[q];
        }
        const int cy = yc[oy * 4 + r];
        acc[0] += h[0] * cy; acc[1] += h[1] * cy; acc[2] += h[2] * cy;
    }
    store_pixel<NHWC4>(acc, dst, dst_u8, i, (int)t, rem, per, m0, m1, m2, s0, s1, s2);
}

}  // namespace

// frames u8 [T][H0][W0][3] RGB (device) -> out f32: layout 0 = NCHW [T][3][out_h][out_w] (the reference's tensor), layout 1 =
// NHWC padded to 4 channels [T][out_h][out_w][4] (what the stem convolution of this implementation stages: skips the
// NCHW -> NHWC4 pass).  The top crop_top rows are dropped, flip != 0 mirrors left-right before resampling.
// xi/xc: [out_w][4] source columns (int32, clamped) and 11-bit taps (int16, each saturate_cast<short>(c * 2048): sum 2047..2049); yi/yc the same for rows of the CROPPED
// image.  out_u8 (optional) [T][out_h][out_w][3]: the resized 8-bit image (what the reference's `img_rgb` holds, x255).
PHNET_API int phnet_preprocess_u8(const uint8_t* frames, float* out, uint8_t* out_u8,
                                  const int32_t* xi, const int16_t* xc, const int32_t* yi, const int16_t* yc,
                                  int32_t T, int32_t H0, int32_t W0, int32_t crop_top, int32_t out_h, int32_t out_w, int32_t flip,
                                  int32_t layout, const float* mean3_host, const float* std3_host, void* stream)
{
    if (T < 0 || H0 < 1 || W0 < 1 || crop_top < 0 || crop_top >= H0 || out_h < 1 || out_w < 1 || (layout != 0 && layout != 1))
        return PHNET_ERR_ARG;
    if (T == 0) return PHNET_OK;
    if (!frames || !out || !xi || !xc || !yi || !yc || !mean3_host || !std3_host) return PHNET_ERR_ARG;
    if (std3_host[0] == 0.f || std3_host[1] == 0.f || std3_host[2] == 0.f) return PHNET_ERR_ARG;
    const long total = (long)T * out_h * out_w;
    const dim3 grid((unsigned)ceil_div64(total, NT));
    if (layout == 1)
        hipLaunchKernelGGL(preprocess_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, frames, out, out_u8, xi, xc, yi, yc, T, H0, W0,
                           crop_top, out_h, out_w, flip, mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0], std3_host[1], std3_host[2]);
    else
        hipLaunchKernelGGL(preprocess_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, frames, out, out_u8, xi, xc, yi, yc, T, H0, W0,
                           crop_top, out_h, out_w, flip, mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0], std3_host[1], std3_host[2]);
    return phnet_launch_status();
}

// frames u8: T camera surfaces frame_stride bytes apart (device).  format 0 = NV12: H0 luma rows of `pitch` bytes, then from
// chroma_offset on H0/2 interleaved U,V rows of `pitch` bytes;  format 1 = YUYV: H0 rows of `pitch` bytes Y0 U Y1 V.  A source
// pixel's colour is c = clamp((m[c][0] (Y - y0) + m[c][1] (U - 128) + m[c][2] (V - 128) + 2^19) >> 20, 0, 255) in int32 with
// csc_host = {y0, m[3][3]} (HOST pointer; rows R, G, B), its chroma the one of the 2x2 (NV12) / 2x1 (YUYV) cell it lies in.  Everything
// after that - tables, crop, flip, taps, rounding, normalisation, layouts, out_u8 - is phnet_preprocess_u8 on those 8-bit colours,
// bit for bit.  Bytes beyond W0 (2 W0) of a row and rows beyond H0 of a plane are never read.
PHNET_API int phnet_preprocess_yuv(const uint8_t* frames, float* out, uint8_t* out_u8,
                                   const int32_t* xi, const int16_t* xc, const int32_t* yi, const int16_t* yc,
                                   int32_t T, int32_t H0, int32_t W0, int32_t crop_top, int32_t out_h, int32_t out_w, int32_t flip,
                                   int32_t layout, int32_t format, int64_t frame_stride, int32_t pitch, int64_t chroma_offset,
                                   const int32_t* csc_host, const float* mean3_host, const float* std3_host, void* stream)
{
    if (T < 0 || H0 < 1 || W0 < 1 || crop_top < 0 || crop_top >= H0 || out_h < 1 || out_w < 1 || (layout != 0 && layout != 1))
        return PHNET_ERR_ARG;
    if ((format != 0 && format != 1) || (W0 & 1) || (format == 0 && (H0 & 1))) return PHNET_ERR_ARG;
    if (pitch < (format == 0 ? 1 : 2) * (int64_t)W0) return PHNET_ERR_ARG;
    if (format == 0 && chroma_offset < (int64_t)pitch * H0) return PHNET_ERR_ARG;
    // the last byte a frame owns: frames closer together than that would overlap
    const int64_t extent = format == 0 ? chroma_offset + (int64_t)(H0 / 2 - 1) * pitch + W0 : (int64_t)(H0 - 1) * pitch + 2 * (int64_t)W0;
    if (frame_stride < extent || extent >= INT32_MAX) return PHNET_ERR_ARG;
    const int64_t per = (int64_t)out_h * out_w, bpf = ceil_div64(per, NT);
    if (per >= INT32_MAX || (int64_t)T * bpf >= INT32_MAX) return PHNET_ERR_ARG;
    if (T == 0) return PHNET_OK;
    if (!frames || !out || !xi || !xc || !yi || !yc || !csc_host || !mean3_host || !std3_host) return PHNET_ERR_ARG;
    if (std3_host[0] == 0.f || std3_host[1] == 0.f || std3_host[2] == 0.f) return PHNET_ERR_ARG;
    Csc k;
    if (!phnet_csc_from_host(csc_host, k)) return PHNET_ERR_ARG;
    const unsigned bpf32 = (unsigned)bpf, pitch32 = (unsigned)pitch, chroma32 = format == 0 ? (unsigned)chroma_offset : 0u;
    const dim3 grid((unsigned)(T * bpf));                          // bpf workgroups per frame: a workgroup never straddles two frames
    const float m0 = mean3_host[0], m1 = mean3_host[1], m2 = mean3_host[2], s0 = std3_host[0], s1 = std3_host[1], s2 = std3_host[2];
    // one load per chroma pair / per YUYV cell needs every address of it aligned: base, frame stride, pitch (and the UV plane's offset)
    const uint64_t low = (uint64_t)(uintptr_t)frames | (uint64_t)frame_stride | (uint64_t)pitch | (format == 0 ? (uint64_t)chroma_offset : 0);
    const bool wide = (low & (format == 0 ? 1 : 3)) == 0;
#define PHNET_YUV_LAUNCH(L, F, W)                                                                                                      \
    hipLaunchKernelGGL((preprocess_yuv_kernel<L, F, W>), grid, dim3(NT), 0, (hipStream_t)stream, frames, out, out_u8, xi, xc, yi, yc, T, bpf32, W0, \
                       crop_top, out_h, out_w, flip, (long)frame_stride, pitch32, chroma32, k, m0, m1, m2, s0, s1, s2)
#define PHNET_YUV_PICK(L, F) do { if (wide) PHNET_YUV_LAUNCH(L, F, true); else PHNET_YUV_LAUNCH(L, F, false); } while (0)
    if (layout == 1) { if (format == 1) PHNET_YUV_PICK(true, true); else PHNET_YUV_PICK(true, false); }
    else             { if (format == 1) PHNET_YUV_PICK(false, true); else PHNET_YUV_PICK(false, false); }
#undef PHNET_YUV_PICK
#undef PHNET_YUV_LAUNCH
    return phnet_launch_status();
}
