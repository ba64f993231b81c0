// What the two three-taps weight-gradient kernels have in common: conv_wgrad3x3_kernel (conv_wgrad.hip, all twelve waves stage)
// and wgrad3s_kernel (wgrad3s.hip, four extra producer waves stage).  Both run one workgroup per (64 co) x (64 ci) x (filter row),
// stage dY[BKW px][64 co] and X[BKW + 2 px][64 ci] as bf16 planes per K step, and twelve waves - tap group dx = wave / 4 - 1,
// quadrant wave % 4 - multiply 32x32 blocks out of them.  Shared here: the LDS image, the tile decode, and the consumer side
// (accumulator start, fragment reads, border mask, epilogue).  The staging and the sub-step loops stay with each kernel, and so
// do the 16-element loop around wgrad3_acc_start and the column step (ke / mx) around wgrad3_mask_edge: with those two inside
// helpers hipcc lays both kernels out differently (other block order, 1-3 more registers), with them outside the kernels keep
// their size and register counts and differ from before in the order of a few scalar instructions of the prologue.
// Internal, not part of the C-ABI.
#pragma once
#include "igemm.h"

namespace {

using namespace igemm;

// LDS image of one operand of a K step of BKW pixels
template <int BKW> struct Wgrad3Image {
    static constexpr int ROWS = BKW + 2;                     // X rows of a step: pixels pt-1 .. pt+BKW of the shifted image row
    static constexpr int PITCH = KStridedPlanes<64, BK>::PITCH;      // 192 bytes: 64 bf16 + pad (igemm.h)
    static constexpr int PLANE = ROWS * PITCH, IMG = 3 * PLANE;      // both operands use the ROWS-row image (dY leaves two rows unused)
};

// the workgroup's tile of dW [Co][3][3][Ci]: output channels m0 .. m0 + 63, filter row dyi, input channels c0 .. c0 + 63
struct Wgrad3Tile {
    int dyi, dy;                         // filter row 0..2, and as an offset -1..1
    int ct, m0, c0;                      // input-channel tile; first output / input channel
};
__device__ __forceinline__ Wgrad3Tile wgrad3_tile(unsigned block, unsigned nblocks, int Ci)
{
    Wgrad3Tile t;
    const int ctiles = Ci >> 6;
    const unsigned tile = xcd_remap(block, nblocks);
    t.dyi = (int)(tile % 3); t.ct = (int)((tile / 3) % ctiles);
    const int mt = (int)(tile / (3 * ctiles));
    t.m0 = mt * 64; t.c0 = t.ct * 64; t.dy = t.dyi - 1;
    return t;
}
// a multiplying wave's 32x32 block of it (waves 0-11: tap group wave / 4, quadrant wave % 4)
struct Wgrad3Wave {
    int tg, dx;                          // tap group 0..2, and as an offset -1..1
    int wm, wn;                          // the quadrant's first row and column in the 64x64 tile
};
__device__ __forceinline__ Wgrad3Wave wgrad3_wave(int wave)
{
    Wgrad3Wave w;
    w.tg = wave >> 2; w.dx = w.tg - 1;
    w.wm = ((wave >> 1) & 1) * 32; w.wn = (wave & 1) * 32;
    return w;
}
// first column of the wave's block in [Co][9 Ci]
__device__ __forceinline__ int wgrad3_n_base(const Wgrad3Tile& t, const Wgrad3Wave& w, int Ci) { return (t.dyi * 3 + w.tg) * Ci + t.c0 + w.wn; }

// what accumulator element e of the block at (row0, n_base) starts from: the old dW when the launch is unsplit and accumulates
// (out is dW then), else zero
__device__ __forceinline__ float wgrad3_acc_start(const float* out, bool from_old, int row0, int n_base, int NC, int lane, int e)
{
    const int n = n_base + frag_col(lane), m = row0 + frag_row(lane, e);
    const float v = out[from_old ? (size_t)m * NC + n : 0];
    return from_old ? v : 0.f;
}

// the wave's dY and X fragments of 16-pixel sub-step ks out of the staged images at a_src / b_src
template <int PITCH, int PLANE>
__device__ __forceinline__ void wgrad3_read_frags(const unsigned char* a_src, const unsigned char* b_src, int lane, int ks, Frag3& a, Frag3& b)
{
    Frag3 (&a1)[1] = *reinterpret_cast<Frag3 (*)[1]>(&a);
    Frag3 (&b1)[1] = *reinterpret_cast<Frag3 (*)[1]>(&b);
    read_kstrided3<1, PITCH, PLANE>(a_src, lane, ks, a1);
    read_kstrided3<1, PITCH, PLANE>(b_src, lane, ks, b1);
}

// clears, in a dY fragment, pixel ke of its 16-pixel block - the one whose tap dx leaves the image row (this lane holds
// k = h8 .. h8 + 7, h8 = (lane >> 5) * 8).  Under a wave-uniform branch: the dx = 0 group never needs it, the others once per
// image row (built unconditionally, these ~26 vector instructions per sub-step ate what the shared staging saves)
__device__ __forceinline__ void wgrad3_mask_edge(Frag3& a, int ke, int h8)
{
    const int j = ke - h8;
    const int ji = j >> 1;                            // register of the element (other half wave: none)
    const unsigned wmask = (j & 1) ? 0x0000ffffu : 0xffff0000u;
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 m;
    m.x = ji == 0 ? wmask : 0xffffffffu; m.y = ji == 1 ? wmask : 0xffffffffu;
    m.z = ji == 2 ? wmask : 0xffffffffu; m.w = ji == 3 ? wmask : 0xffffffffu;
    a.hi = __builtin_bit_cast(bf16x8, __builtin_bit_cast(u32x4, a.hi) & m);
    a.mid = __builtin_bit_cast(bf16x8, __builtin_bit_cast(u32x4, a.mid) & m);
    a.lo = __builtin_bit_cast(bf16x8, __builtin_bit_cast(u32x4, a.lo) & m);
}

// stores the block at (row0, n_base) into dW (splits == 1) or into row `split` of the partial buffer [splits][Co * NC + Co]; returns that row
__device__ __forceinline__ float* wgrad3_store(float* out, int splits, unsigned split, int Co, int NC, int row0, int n_base, int lane,
                                               const f32x16& acc)
{
    float* dst = splits == 1 ? out : out + (size_t)split * ((size_t)Co * NC + Co);
#pragma unroll
    for (int e = 0; e < 16; ++e)
        dst[(size_t)(row0 + frag_row(lane, e)) * NC + n_base + frag_col(lane)] = acc[e];
    return dst;
}

}  // namespace
