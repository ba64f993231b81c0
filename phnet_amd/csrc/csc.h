// The integer Y'CbCr -> 8-bit R'G'B' conversion of the camera formats (NV12, YUYV), shared by every kernel that reads a camera
// surface: preprocess.hip (each bicubic tap) and lane_draw.hip (the pixel under an overlay).  One definition, so the overlay shows
// exactly the colours the network was fed.
#pragma once
#include "common.h"

struct Csc { int bias[3]; int m[9]; };      // 20-bit fixed point, rows R, G, B; columns Y, U, V; bias = 2^19 - m0 y0 - 128 (m1 + m2)

// c = clamp((m0 (Y - y0) + m1 (U - 128) + m2 (V - 128) + 2^19) >> 20, 0, 255) with the constant terms folded into `bias` by the entry:
// the same integer (sums mod 2^32 of a value the entry checked to fit int32), three multiply-adds instead of three subtractions more.
// 24-bit multiplies (full rate; the 32-bit one is quarter rate) are exact here: |m| < 2^23 is checked by the entry, Y, U, V < 2^8.
__device__ __forceinline__ int csc_channel(const Csc& k, int c, int Y, int U, int V)
{
    const unsigned a = (unsigned)k.bias[c] + (unsigned)__mul24(k.m[3 * c], Y) + (unsigned)__mul24(k.m[3 * c + 1], U) + (unsigned)__mul24(k.m[3 * c + 2], V);
    const int q = (int)a >> 20;                                    // arithmetic shift: floors
    return q < 0 ? 0 : (q > 255 ? 255 : q);
}

// csc_host [10] = y0, then m row-major -> k.  false: y0 outside 0..255, a coefficient outside 24 bits, or an accumulator that could
// leave int32 (255 * sum |m| + 2^19 must fit).
static inline bool phnet_csc_from_host(const int32_t* csc_host, Csc& k)
{
    const int y0 = csc_host[0];
    if (y0 < 0 || y0 > 255) return false;
    for (int c = 0; c < 3; ++c) {
        int64_t reach = 1 << 19;                                  // |accumulator| <= 255 * sum |m| + 2^19 must fit int32, a coefficient 24 bits
        for (int j = 0; j < 3; ++j) {
            k.m[3 * c + j] = csc_host[1 + 3 * c + j];
            const int64_t a = k.m[3 * c + j];
            reach += 255 * (a < 0 ? -a : a);
            if (a <= -(1 << 23) || a >= (1 << 23)) return false;
        }
        if (reach > INT32_MAX) return false;
        k.bias[c] = (int)((1u << 19) - (uint32_t)k.m[3 * c] * (uint32_t)y0 - 128u * ((uint32_t)k.m[3 * c + 1] + (uint32_t)k.m[3 * c + 2]));
    }
    return true;
}
