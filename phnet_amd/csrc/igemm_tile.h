// The implicit-GEMM tile program of the forward / data-gradient kernels (conv_igemm.h: conv.hip, linear_bwd.hip) and of the data-gradient
// half of linear_bwd.hip.  Internal, not part of the C-ABI.
#pragma once
#include "conv_common.h"

using namespace igemm;

namespace {

// Block -> tile for the class-ordered rows of a dilated data gradient (DIL below).  xcd_remap hands every XCD ONE run of
// consecutive tiles, which here would be one parity class: the two XCDs that got the four-tap class of a 3x3 filter ran 32 K
// tiles per workgroup while two others ran 8, and the launch took as long as those two.  So the tiles are cut into segments of
// 8 * chunk and only inside a segment does an XCD (block & 7: workgroups go to the XCDs round robin) take a run of `chunk`
// consecutive tiles - every XCD gets the same share of every class, neighbouring tiles still meet in one L2.  Bijective: the
// full segments permute themselves, the remainder goes through xcd_remap.
__device__ __forceinline__ unsigned xcd_remap_striped(unsigned bid, unsigned nblocks) {
    const unsigned chunk = max(1u, min(16u, nblocks >> 6)), seg = 8u * chunk;
    const unsigned full = nblocks / seg * seg;
    if (bid >= full) return full + xcd_remap(bid - full, nblocks - full);
    const unsigned s = bid / seg, w = bid - s * seg;
    return s * seg + (w & 7u) * chunk + (w >> 3);
}

// The tile program is a device function so that one launch can run tiles of different GEMMs (linear_bwd_fused_kernel);
// (block, nblocks, split) are what blockIdx.x / gridDim.x / blockIdx.z are for the plain kernel below.
// AMASK: the A operand is a gradient that still has to pass a ReLU - element (row, k) counts only where amask (the saved
// forward output of that ReLU, same layout as X) is positive; applied when the tile is written to LDS.
// PF: register prefetch depth in K tiles.  The loads of tile t + PF are issued while tile t is multiplied, so PF tiles of a
// workgroup are in flight at any time: at one clip the trunk GEMMs are bound by the latency of their operand loads times
// the little that is in flight per CU (measured: 9 B/clk/CU at PF = 1 against the ~28 B/clk/CU an L2-resident gather
// sustains, MI355X_MICROARCH.md "Indexed rows"), not by the MFMA pipe - which is why the 2.7x cheaper bf16x3 arithmetic
// alone changed nothing.  A tile costs 2-4 float4 registers per thread, the LDS double buffer stays.
// BUF: operand loads through buffer instructions with 32-bit offsets (uniform-tap, undilated, unmasked-A problems only): an
// out-of-range element is simply given an offset past the end of the tensor and the hardware returns zeros - no 64-bit
// address arithmetic, no validity select when the tile is written to LDS (the loop is bound by its vector instruction
// count: 90 per 6 MFMAs before, of which 44 are the split).
// MMA: the arithmetic (igemm.h) - 0 f32-input MFMA, 1 / 2 bf16 splits in registers (f32 LDS images), 3 the exact split staged as
// three bf16 planes, 4 the bf16 inference arithmetic: ONE staged bf16 plane per operand, one MFMA per product (forward launches only;
// staging, ring, buffer loads and epilogues are mode 3's).
// DIL (needs B_DGRAD && UNI && !BUF; the caller guarantees g.in_dil == 2 and a filter of at most 16 taps, R, S <= 16:
// conv_igemm_kernel branches to this instantiation at run time and keeps the plain one for every other problem): the data
// gradient of a stride-2 convolution gathers from a dY image dilated by 2, so a dX pixel of parity class (y & 1, x & 1) can use
// only the taps with r = (y + pad) mod 2, q = (x + pad) mod 2 - 1, 2, 2 or 4 of the 9 of a 3x3 / pad 1 filter, one class of four
// for a 1x1 - and the other A rows used to be staged as zeros and multiplied.  Here the GEMM rows list the pixels class by class
// (the class with the most live taps first; inside a class by (n, y >> 1, x >> 1)), so that a tile's rows share their live
// taps, and the scalar tap walk visits only the taps of the classes the tile holds: its K extent is (live taps) x Ci, each
// split walking the part of it that lies in its range of the full K; a tile without a live tap runs no K tile.  The per-row
// parity test of the A loads stays, so a tile that holds several classes merely skips less.  Grid, tile count, split-K slabs
// (indexed by the real pixel) and the reduce are untouched.
template <int BM, int BN, bool B_DGRAD, int BKT, bool UNI, bool AMASK = false, int MMA = 0, int PF = 1, bool BUF = false,
          bool DIL = false>
__device__ __forceinline__ void igemm_tile(
    const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias,
    const float* __restrict__ addend, float* __restrict__ out, const ConvShape& g, int relu,
    float* lds, unsigned block, unsigned nblocks, unsigned split, const float* __restrict__ amask = nullptr,
    float* __restrict__ stats = nullptr)
{
    constexpr int TM = BM / 2, TN = BN / 2, FM = TM / 32, FN = TN / 32;
    constexpr int A_PITCH = KContigTile<BM, BKT>::PITCH;
    constexpr int A_FLOATS = KContigTile<BM, BKT>::FLOATS;
    constexpr int B_PITCH = B_DGRAD ? KStridedTile<BN, BKT>::PITCH : KContigTile<BN, BKT>::PITCH;
    constexpr int B_FLOATS = B_DGRAD ? KStridedTile<BN, BKT>::FLOATS : KContigTile<BN, BKT>::FLOATS;
    constexpr int CHUNKS = BKT / 4;                         // float4 chunks along K per row
    constexpr int ROWS_PER_PASS = THREADS / CHUNKS;         // 64 (BKT 16) or 16 (BKT 64)
    constexpr int A_LOADS = BM / ROWS_PER_PASS;             // float4 loads per thread per K tile
    constexpr int B_LOADS = B_DGRAD ? (BKT * BN / 4) / THREADS : BN / ROWS_PER_PASS;
    float* As = lds;
    float* Bs = lds + 2 * A_FLOATS;
    // MMA = 3: bf16 planes instead of f32 images (igemm.h)
    // MMA = 4: ONE bf16 plane per operand (the bf16 inference arithmetic, igemm.h) - same pitches, same offsets inside a plane
    constexpr bool S3 = MMA == 3, S1 = MMA == 4;
    constexpr int NP = S1 ? 1 : 3;
    typedef KContigPlanes<BM, BKT, NP> AP3;
    typedef KContigPlanes<BN, BKT, NP> BP3C;
    typedef KStridedPlanes<BN, BKT, NP> BP3S;
    constexpr int B3_BYTES = B_DGRAD ? BP3S::BYTES : BP3C::BYTES;
    unsigned char* A3 = reinterpret_cast<unsigned char*>(lds);
    unsigned char* B3 = A3 + 2 * AP3::BYTES;

    const int M = g.N * g.Ho * g.Wo;
    const int K = g.R * g.S * g.Ci;
    const int tiles_n = (g.Co + BN - 1) / BN;
    const unsigned tile = DIL ? xcd_remap_striped(block, nblocks) : xcd_remap(block, nblocks);
    const int m0 = (int)(tile / tiles_n) * BM, n0 = (int)(tile % tiles_n) * BN;
    int k_begin = split * g.k_per_split;
    int k_end = min(K, k_begin + g.k_per_split);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * TM, wn = (wave & 1) * TN;

    // ---- DIL: the pixel of each of the tile's rows (-1 past M), the tile's live taps, its share of their K tiles ----
    unsigned long long tap_rs = 0, tap_qs = 0;             // the live taps in walking order, a nibble each
    int tap_ord = 0;                                        // position of the walk in that list
    int* row_pix = nullptr;
    if constexpr (DIL) {
        static_assert(B_DGRAD && UNI && !BUF && BM <= THREADS, "dilated data gradient: uniform tap, plain loads");
        __shared__ int pix_s[BM];
        row_pix = pix_s;
        // order of the classes: c = 2 a + b holds the pixels with y & 1 == a ^ fy, x & 1 == b ^ fx; fy / fx put the parity
        // with more live filter rows / columns first (an even coordinate starts at tap pad & 1, an odd one at the other)
        const int e0 = g.pad & 1, o0 = e0 ^ 1;
        const int fy = (g.R - o0 + 1) / 2 > (g.R - e0 + 1) / 2, fx = (g.S - o0 + 1) / 2 > (g.S - e0 + 1) / 2;
        const int h0 = fy ? g.Ho >> 1 : (g.Ho + 1) >> 1, h1 = g.Ho - h0;         // image rows / columns of a = 0, 1 and b = 0, 1
        const int w0 = fx ? g.Wo >> 1 : (g.Wo + 1) >> 1, w1 = g.Wo - w0;
        const int cs1 = g.N * h0 * w0, cs2 = cs1 + g.N * h0 * w1, cs3 = cs2 + g.N * h1 * w0;      // first row of classes 1, 2, 3
        const int m_hi = min(m0 + BM, M);
        const unsigned held = (unsigned)(max(0, m0) < min(cs1, m_hi)) | (unsigned)(max(cs1, m0) < min(cs2, m_hi)) << 1 |
                              (unsigned)(max(cs2, m0) < min(cs3, m_hi)) << 2 | (unsigned)(max(cs3, m0) < min(M, m_hi)) << 3;
        // K as this tile walks it: (live taps) x Ci.  A split keeps the K tiles the host's cut of the FULL K gave it ([k_begin, k_end)
        // so far) and walks the live ones among them - a run of the walk, since both orders are (r, q, c) - so every slab holds
        // the partial sum it always held, bit for bit (the skipped products were exact zeros); a split whose range holds no live
        // tile writes zeros.  (Dividing the live K tiles evenly instead regroups the sums of a 4-split launch: 6e-7 of the
        // gradient, which 25 AdamW steps of bench.py turn into another loss.)
        int live = 0, walk_begin = 0, walk_end = 0;     // tap (r, q) serves exactly one class
        for (int r = 0; r < g.R; ++r)
            for (int q = 0; q < g.S; ++q) {
                const int c = 2 * (((r + g.pad) & 1) ^ fy) + (((q + g.pad) & 1) ^ fx);
                if ((held >> c) & 1u) {
                    tap_rs |= (unsigned long long)r << (4 * live);
                    tap_qs |= (unsigned long long)q << (4 * live);
                    ++live;
                    const int k_tap = (r * g.S + q) * g.Ci;                  // where the tap starts in the full K
                    walk_begin += min(max(k_begin - k_tap, 0), g.Ci);
                    walk_end += min(max(k_end - k_tap, 0), g.Ci);
                }
            }
        k_begin = walk_begin;
        k_end = walk_end;
        const int j = m0 + tid;
        const int c = (j >= cs1) + (j >= cs2) + (j >= cs3);
        const int l = j - (c == 0 ? 0 : c == 1 ? cs1 : c == 2 ? cs2 : cs3);
        const int hc = (c >> 1) ? h1 : h0, wc = (c & 1) ? w1 : w0, hw = max(hc * wc, 1);
        const int n = l / hw, rem = l - n * hw, yh = rem / max(wc, 1), xh = rem - yh * wc;
        const int pixel = (n * g.Ho + 2 * yh + ((c >> 1) ^ fy)) * g.Wo + 2 * xh + ((c & 1) ^ fx);
        if (tid < BM) pix_s[tid] = m0 + tid < M ? pixel : -1;
        __syncthreads();
    }

    // ---- per-thread gather coordinates of the A rows this thread stages (fixed over the K loop) ----
    RowCoord rc[A_LOADS];
    const int a_chunk = tid % CHUNKS, a_row = tid / CHUNKS;
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i) {
        int m = m0 + a_row + ROWS_PER_PASS * i;
        rc[i].ok = m < M;
        if constexpr (DIL) m = row_pix[a_row + ROWS_PER_PASS * i];
        const int mm = rc[i].ok ? m : 0;
        const int n = mm / (g.Ho * g.Wo), rem = mm - n * (g.Ho * g.Wo);
        const int oy = rem / g.Wo, ox = rem - oy * g.Wo;
        rc[i].base = n * g.Hi * g.Wi;
        rc[i].iy0 = oy * g.stride - g.pad;
        rc[i].ix0 = ox * g.stride - g.pad;
    }

    // ---- running (tap, channel) decomposition of this thread's k index: one division at start-up, then
    // carry-propagating adds per K tile (per-step integer divisions made the loop VALU-bound) ----------
    struct KPos { int c, r, q; };
    auto kpos_init = [&](int k, int ci) {
        KPos p;
        const int rs = k / ci;
        p.c = k - rs * ci;
        p.r = rs / g.S;
        p.q = rs - p.r * g.S;
        return p;
    };
    auto kpos_advance = [&](KPos& p, int ci) {
        p.c += BKT;
        while (p.c >= ci) {
            p.c -= ci;
            if (++p.q == g.S) { p.q = 0; ++p.r; }
        }
    };
    KPos ka = kpos_init(k_begin + a_chunk * 4, g.Ci);
    KPos kb[B_LOADS];
    int b_kk[B_LOADS], b_ch[B_LOADS];
    if (B_DGRAD) {
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i) {
            const int idx = tid + THREADS * i;                     // BKT rows x BN/4 chunks
            b_kk[i] = idx / (BN / 4);
            b_ch[i] = idx - b_kk[i] * (BN / 4);
            kb[i] = kpos_init(k_begin + b_kk[i], g.Ci);
        }
    }

    // Uniform-tap fast path: when the A-side channel count is a multiple of the K tile, every K tile lies inside ONE filter
    // tap (r,q), the same for the whole workgroup, so the tap walks in scalar registers and a thread's address math per
    // tile is a handful of VALU ops (the general path below carries a per-thread (c,r,q) decomposition and made the
    // trunk loops VALU-bound: ~190 instructions per 8 MFMAs).
    constexpr bool uni = UNI;                            // host guarantees g.Ci % BKT == 0
    int ur = 0, uq = 0, uc0 = 0;
    if (uni) {
        const int rs = k_begin / g.Ci;
        uc0 = k_begin - rs * g.Ci;
        ur = rs / g.S;
        uq = rs - ur * g.S;
        if constexpr (DIL) {                             // rs counts live taps here
            tap_ord = min(rs, 15);
            ur = (int)(tap_rs >> (4 * tap_ord)) & 15;
            uq = (int)(tap_qs >> (4 * tap_ord)) & 15;
        }
    }

    // The loads are BRANCH-FREE: an out-of-range element reads element 0 of its array and is zeroed when it is written to
    // LDS (validity bits travel in `mask`: A loads in bits 0.., B loads in bits 16..), so the loop body is straight-line
    // code the compiler can schedule and count (s_waitcnt) exactly.  (A second register set prefetching two tiles ahead
    // was measured too: +4 % on the trunk forward, -3 % on the skinny head GEMMs, no gain on the step - not kept.)
    f32x4 a_set[PF][A_LOADS], b_set[PF][B_LOADS];
    f32x4 r_set[PF][AMASK ? A_LOADS : 1];
    unsigned mask_set[PF];
    // loads the K tile that starts at kt; MUST be called with kt = k_begin, k_begin+BKT, ... in order
    // ---- BUF: per-thread byte offsets fixed over the K loop + one scalar offset per tile ----
    constexpr unsigned OOB = 0x80000000u;                 // past the end of every tensor of this path (< 2 GB each)
    int a_off[BUF ? A_LOADS : 1], b_off[BUF ? B_LOADS : 1];
    __amdgpu_buffer_rsrc_t x_rsrc, w_rsrc;
    if constexpr (BUF) {
        static_assert(UNI && !AMASK, "buffer-load path: uniform tap, no ReLU mask");
        x_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)X, 0, (int)min((long)g.N * g.Hi * g.Wi * g.Ci * 4, (long)0x7fffffff), 0x00020000);
        w_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)W, 0, (int)min((long)g.Co * K * 4, (long)0x7fffffff), 0x00020000);
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) {
            a_off[i] = ((rc[i].base + rc[i].iy0 * g.Wi + rc[i].ix0) * g.Ci + a_chunk * 4) * 4;
            if (!rc[i].ok) rc[i].iy0 = -(1 << 28);                       // fails the row test below for every tap
        }
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i) {
            if (!B_DGRAD) {
                const int n = n0 + a_row + ROWS_PER_PASS * i;
                b_off[i] = n < g.Co ? (n * K + a_chunk * 4) * 4 : (int)OOB;
            } else {
                const int n = n0 + b_ch[i] * 4;
                b_off[i] = n < g.Co ? (b_kk[i] * g.R * g.S * g.Co + n) * 4 : (int)OOB;
            }
        }
    }
    auto load_global = [&](int kt, f32x4 (&a_reg)[A_LOADS], f32x4 (&b_reg)[B_LOADS], f32x4 (&a_relu)[AMASK ? A_LOADS : 1], unsigned& mask) {
        mask = 0;
        if constexpr (BUF) {
            const bool tile_ok = kt < k_end;                             // uniform: K and the split bounds are multiples of BKT
            const int s_tap = ((ur * g.Wi + uq) * g.Ci + uc0) * 4;
#pragma unroll
            for (int i = 0; i < A_LOADS; ++i) {
                const bool ok = tile_ok && (unsigned)(rc[i].iy0 + ur) < (unsigned)g.Hi && (unsigned)(rc[i].ix0 + uq) < (unsigned)g.Wi;
                a_reg[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, ok ? a_off[i] + s_tap : (int)OOB, 0, 0));
            }
            // B: scalar part of the offset
            int s_b;
            if (!B_DGRAD) s_b = kt * 4;
            else s_b = ((uc0 * g.R + (g.R - 1 - ur)) * g.S + (g.S - 1 - uq)) * g.Co * 4;
#pragma unroll
            for (int i = 0; i < B_LOADS; ++i)            // (an invalid column already sits at OOB; adding the small s_b keeps it there)
                b_reg[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, tile_ok ? b_off[i] + s_b : (int)OOB, 0, 0));
            uc0 += BKT;
            const int wc = uc0 >= g.Ci;
            uc0 = wc ? 0 : uc0;
            uq += wc;
            const int wq = uq == g.S;
            uq = wq ? 0 : uq;
            ur += wq;
            return;
        }
        // A: CHUNKS consecutive lanes fetch BKT*4 contiguous bytes of one pixel tap
        const int k0 = kt + a_chunk * 4;
        const bool kok = k0 < k_end;
        const int tap_r = uni ? ur : ka.r, tap_q = uni ? uq : ka.q, tap_c = uni ? uc0 + a_chunk * 4 : ka.c;
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) {
            int ty = rc[i].iy0 + tap_r, tx = rc[i].ix0 + tap_q;
            bool ok = kok && rc[i].ok && ty >= 0 && tx >= 0;
            if (g.in_dil == 2) {                        // dgrad of a stride-2 conv (strides > 2 are rejected on the host)
                ok = ok && !((ty | tx) & 1);
                ty >>= 1; tx >>= 1;
            }
            ok = ok && ty < g.Hi && tx < g.Wi;
            const int pix = ok ? rc[i].base + ty * g.Wi + tx : 0;         // masked: pixel 0 (valid memory, value discarded)
            a_reg[i] = *reinterpret_cast<const f32x4*>(X + (size_t)pix * g.Ci + (kok ? tap_c : 0));
            if (AMASK) a_relu[i] = *reinterpret_cast<const f32x4*>(amask + (size_t)pix * g.Ci + (kok ? tap_c : 0));
            mask |= (unsigned)ok << i;
        }
        if (!uni) kpos_advance(ka, g.Ci);
        if (!B_DGRAD) {
            // B rows = output channels, K contiguous in the OHWI weight
#pragma unroll
            for (int i = 0; i < B_LOADS; ++i) {
                const int n = n0 + a_row + ROWS_PER_PASS * i;
                const bool ok = kok && n < g.Co;
                b_reg[i] = *reinterpret_cast<const f32x4*>(W + (size_t)(ok ? n : 0) * K + (kok ? k0 : 0));
                mask |= (unsigned)ok << (16 + i);
            }
        } else {
            // B rows = k = (r,q,co) of the dgrad sum; columns = ci, contiguous in W[co][R-1-r][S-1-q][:]
            // here g.Ci is the dY channel count (= weight Co) and g.Co the weight Ci
#pragma unroll
            for (int i = 0; i < B_LOADS; ++i) {
                const int k = kt + b_kk[i], n = n0 + b_ch[i] * 4;
                const bool ok = k < k_end && n < g.Co;
                const int wc = uni ? uc0 + b_kk[i] : kb[i].c, wr = uni ? ur : kb[i].r, wq = uni ? uq : kb[i].q;
                const int wrow = ok ? (wc * g.R + (g.R - 1 - wr)) * g.S + (g.S - 1 - wq) : 0;
                b_reg[i] = *reinterpret_cast<const f32x4*>(W + (size_t)wrow * g.Co + (ok ? n : 0));
                mask |= (unsigned)ok << (16 + i);
                if (!uni) kpos_advance(kb[i], g.Ci);
            }
        }
        if (uni) {                                       // scalar tap walk, branch-free (a branch here costs a vmcnt(0))
            uc0 += BKT;
            const int wc = uc0 >= g.Ci;
            uc0 = wc ? 0 : uc0;
            uq += wc;
            const int wq = uq == g.S;
            uq = wq ? 0 : uq;
            ur += wq;
            if constexpr (DIL) {                         // the next live tap (past the last one: tap 0, the loads are masked by k_end)
                tap_ord = min(tap_ord + wc, 15);
                ur = (int)(tap_rs >> (4 * tap_ord)) & 15;
                uq = (int)(tap_qs >> (4 * tap_ord)) & 15;
            }
        }
    };
    auto store_lds = [&](int buf, const f32x4 (&a_reg)[A_LOADS], const f32x4 (&b_reg)[B_LOADS], const f32x4 (&a_relu)[AMASK ? A_LOADS : 1],
                         unsigned mask) {
        float* a = As + buf * A_FLOATS;
        float* b = Bs + buf * B_FLOATS;
        unsigned char* a3 = A3 + buf * AP3::BYTES;
        unsigned char* b3 = B3 + buf * B3_BYTES;
        const f32x4 zero{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) {
            f32x4 v = BUF ? a_reg[i] : ((mask >> i) & 1u ? a_reg[i] : zero);
            if (AMASK) {
                v.x = a_relu[i].x > 0.f ? v.x : 0.f; v.y = a_relu[i].y > 0.f ? v.y : 0.f;
                v.z = a_relu[i].z > 0.f ? v.z : 0.f; v.w = a_relu[i].w > 0.f ? v.w : 0.f;
            }
            if (S3) store_split3<AP3::PLANE>(a3, (a_row + ROWS_PER_PASS * i) * AP3::PITCH + a_chunk * 8, v);
            else if (S1) store_bf16(a3, (a_row + ROWS_PER_PASS * i) * AP3::PITCH + a_chunk * 8, v);
            else
            *reinterpret_cast<f32x4*>(a + (a_row + ROWS_PER_PASS * i) * A_PITCH + a_chunk * 4) = v;
        }
        if (!B_DGRAD) {
#pragma unroll
            for (int i = 0; i < B_LOADS; ++i) {
                const f32x4 v = BUF ? b_reg[i] : ((mask >> (16 + i)) & 1u ? b_reg[i] : zero);
                if (S3) store_split3<BP3C::PLANE>(b3, (a_row + ROWS_PER_PASS * i) * BP3C::PITCH + a_chunk * 8, v);
                else if (S1) store_bf16(b3, (a_row + ROWS_PER_PASS * i) * BP3C::PITCH + a_chunk * 8, v);
                else *reinterpret_cast<f32x4*>(b + (a_row + ROWS_PER_PASS * i) * B_PITCH + a_chunk * 4) = v;
            }
        } else {
#pragma unroll
            for (int i = 0; i < B_LOADS; ++i) {
                const f32x4 v = BUF ? b_reg[i] : ((mask >> (16 + i)) & 1u ? b_reg[i] : zero);
                if (S3) store_split3<BP3S::PLANE>(b3, b_kk[i] * BP3S::PITCH + b_ch[i] * 8, v);
                else if (S1) store_bf16(b3, b_kk[i] * BP3S::PITCH + b_ch[i] * 8, v);
                else *reinterpret_cast<f32x4*>(b + b_kk[i] * B_PITCH + b_ch[i] * 4) = v;
            }
        }
    };

    // unsplit launches start their accumulators from bias (+ addend): those reads overlap the first K tile's loads and the
    // epilogue has no loads left (16 dependent global reads per fragment, each waited for, when the addend sat there)
    const bool final_pass = g.splits == 1;
    f32x16 acc[FM][FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int n = n0 + wn + j * 32 + frag_col(lane);
        const bool nok = n < g.Co;
        const float bv = (final_pass && bias && nok) ? bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                int m = m0 + wm + i * 32 + frag_row(lane, e);
                if constexpr (DIL) m = row_pix[wm + i * 32 + frag_row(lane, e)];
                const bool ok = final_pass && addend && nok && (DIL ? m >= 0 : m < M);
                acc[i][j][e] = bv + (ok ? addend[(size_t)(ok ? m : 0) * g.Co + (ok ? n : 0)] : 0.f);
            }
    }

    auto multiply_tile = [&](int buf, int kt) {
        if (S3) {
            // no early exit on a ragged K tail here: ds_read_b64_tr_b16 needs every lane (the tail of the tile is zeros)
#pragma unroll
            for (int ks = 0; ks < BKT / BK; ++ks) {
                Frag3 a[FM], b[FN];
                read_kcontig3<FM, AP3::PITCH, AP3::PLANE>(A3 + buf * AP3::BYTES + wm * AP3::PITCH, lane, ks, a);
                if (!B_DGRAD) read_kcontig3<FN, BP3C::PITCH, BP3C::PLANE>(B3 + buf * B3_BYTES + wn * BP3C::PITCH, lane, ks, b);
                else read_kstrided3<FN, BP3S::PITCH, BP3S::PLANE>(B3 + buf * B3_BYTES + wn * 2, lane, ks, b);
                mma3_step<FM, FN>(a, b, acc);
            }
            return;
        }
        if (S1) {
            // (no early exit on a ragged K tail either: the tail of the tile is staged as zeros)
#pragma unroll
            for (int ks = 0; ks < BKT / BK; ++ks) {
                bf16x8 a[FM], b[FN];
                read_kcontig1<FM, AP3::PITCH>(A3 + buf * AP3::BYTES + wm * AP3::PITCH, lane, ks, a);
                if (!B_DGRAD) read_kcontig1<FN, BP3C::PITCH>(B3 + buf * B3_BYTES + wn * BP3C::PITCH, lane, ks, b);
                else read_kstrided1<FN, BP3S::PITCH>(B3 + buf * B3_BYTES + wn * 2, lane, ks, b);
                mma1_step<FM, FN>(a, b, acc);
            }
            return;
        }
#pragma unroll
        for (int ks = 0; ks < BKT / BK; ++ks) {
            if (BKT > BK && kt + ks * BK >= k_end) break;              // ragged K tail of a deep tile
            float a[FM][8], b[FN][8];
            read_kcontig<FM, A_PITCH>(As + buf * A_FLOATS + wm * A_PITCH, lane, ks, a);
            if (!B_DGRAD) read_kcontig<FN, B_PITCH>(Bs + buf * B_FLOATS + wn * B_PITCH, lane, ks, b);
            else read_kstrided<FN, B_PITCH>(Bs + buf * B_FLOATS + wn, lane, ks, b);
            mma_any<(S3 || S1) ? 0 : MMA, FM, FN>(a, b, acc);
        }
    };

    if (k_begin < k_end) {
        const int ntiles = (k_end - k_begin + BKT - 1) / BKT;
        // ring of PF register sets: slot (t mod PF) holds tile t until it has been written to LDS (one iteration before it is
        // multiplied), then takes tile t + PF.  Loads past the end are fully masked (they read element 0).
#pragma unroll
        for (int d = 0; d < PF; ++d) load_global(k_begin + d * BKT, a_set[d], b_set[d], r_set[d], mask_set[d]);
        store_lds(0, a_set[0], b_set[0], r_set[0], mask_set[0]);
        __syncthreads();
        int buf = 0;
        // one iteration: slot U was emptied an iteration ago and takes tile tt + PF; tile tt (in LDS) is multiplied; tile
        // tt + 1 moves from its slot to the other LDS buffer.  Straight-line code (no branch between the loads and their use:
        // hipcc answers a branch with s_waitcnt vmcnt(0), which would drain the whole ring every iteration).
        auto iteration = [&](auto U, int tt) {
            constexpr int u = decltype(U)::value;
            load_global(k_begin + (tt + PF) * BKT, a_set[u], b_set[u], r_set[u], mask_set[u]);
            multiply_tile(buf, k_begin + tt * BKT);
            // keep the LDS fill (and the wait for the global loads in front of it) BEHIND the MFMAs: left alone, the
            // scheduler hoists it above them - the operands are already in registers - and every wave then sits out its
            // full load latency before it issues a single MFMA
            // (with a deep ring the loads are long since complete: the scheduler is free to interleave the split / LDS fill of
            // the next tile with this tile's MFMAs, which would otherwise leave the vector ALU idle while the matrix pipe drains)
            if (PF == 1) __builtin_amdgcn_sched_barrier(0);
            constexpr int v = (u + 1) % PF;
            store_lds(buf ^ 1, a_set[v], b_set[v], r_set[v], mask_set[v]);
            if (PF > 1 && S3 && g_interleave) {
                // one MFMA, then a handful of the next tile's split / address instructions, ...: the matrix pipe takes an MFMA
                // every 32 cycles and blocks the vector issue for 8 of them
#pragma unroll
                for (int i = 0; i < 6 * FM * FN * (BKT / BK); ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, (14 + FM * FN - 1) / (FM * FN), 0);
                }
            }
            __syncthreads();
            buf ^= 1;
        };
        int t = 0;
        for (; t + PF <= ntiles; t += PF) unroll_iterations<PF>(iteration, t);
        if (PF > 1) tail_iterations<PF - 1>(iteration, t, ntiles);
    }

    // ---- per-channel statistics of the result (BatchNorm's batch statistics without a second pass over the tensor):
    // every 32-row slab of the output writes its (sum, sum of squares) per column into stats[slab][2*Co]; rows past M are
    // exact zeros (their A rows were zero and a convolution in front of a BatchNorm has no bias) -------------------
    if (stats != nullptr && final_pass) {
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            const int n = n0 + wn + j * 32 + frag_col(lane);
#pragma unroll
            for (int i = 0; i < FM; ++i) {
                float sm = 0.f, sq = 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e) { const float v = acc[i][j][e]; sm += v; sq += v * v; }
                sm += __shfl_xor(sm, 32, 64);
                sq += __shfl_xor(sq, 32, 64);
                if (lane < 32 && n < g.Co) {
                    float* p = stats + (size_t)((m0 + wm + i * 32) >> 5) * 2 * g.Co;
                    p[n] = sm;
                    p[g.Co + n] = sq;
                }
            }
        }
    }

    // ---- epilogue: bias / relu, or raw partial sums when split-K --------------------------------
    float* dst = out + (size_t)split * M * g.Co;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int n = n0 + wn + j * 32 + frag_col(lane);
        if (n >= g.Co) continue;
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                int m = m0 + wm + i * 32 + frag_row(lane, e);
                if constexpr (DIL) m = row_pix[wm + i * 32 + frag_row(lane, e)];
                if (DIL ? m >= 0 : m < M) dst[(size_t)m * g.Co + n] = (final_pass && relu) ? fmaxf(acc[i][j][e], 0.f) : acc[i][j][e];
            }
    }
}

}  // namespace
