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
//
// The kernel is the template of csrc/augment_warp.h, instantiated here without its stencil switch.  The neighbourhood ops of the 'complex'
// recipe (rule 7: edge filters and blurs) need a staging pass and live behind phnet_augment_stencil_u8, csrc/augment_stencil.hip.
#include "augment_warp.h"

// frames u8 [T][H][W][3] (device; the out_u8 of phnet_preprocess_u8 / _yuv), out f32 NCHW [T][3][H][W] (layout 0) or NHWC4 [T][H][W][4]
// (layout 1), out_u8 optional [T][H][W][3]; flip2 i32 [T], inv f64 [T][6], table i32 [T][16] on the device; mean3 / std3 HOST pointers.
PHNET_API int phnet_augment_u8(const uint8_t* frames, float* out, uint8_t* out_u8, const int32_t* flip2, const double* inv,
                               const int32_t* table, int32_t T, int32_t H, int32_t W, int32_t layout, const float* mean3_host,
                               const float* std3_host, void* stream)
{
    return augment_launch<false>(frames, out, out_u8, flip2, inv, table, nullptr, nullptr, T, H, W, layout, mean3_host, std3_host, stream);
}
