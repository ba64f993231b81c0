// Weight gradient of the convolutions / Linear layers of conv.hip (same layouts: NHWC activations, OHWI weights):
//   dW[co][r][q][c] = sum_pixels dY[pix][co] * X[pix shifted by (r,q)][c]
//   GEMM  M = Co, N = R*S*Ci, K = pixels (split over blockIdx.z, deterministic 2-pass reduce); both operands K-strided.
// Five kernel families behind one entry point (pick_wgrad): the generic one, the three-taps 3x3 one and the few-rows Linear one
// here, the two producer / consumer ones in wgrad3s.hip and wgrad1s.hip (wgrad_pc.h).
#include <cstdio>
#include "conv_common.h"
#include "smallp_tile.h"
#include "wgrad3_taps.h"
#include "tuning.h"
#include "wgrad_pc.h"

using namespace igemm;

namespace {

// out: dW itself when g.splits == 1 (written or accumulated in the epilogue) else the split-K partial buffer
// [splits][Co*NC + Co] (the trailing Co floats of every split hold its bias-gradient partial).
// PF / BUF: register prefetch ring and buffer loads as in igemm_tile (used by the staged-split arithmetic)
template <int BM, int BN, int MMA = 0, int BKW = BK, int PF = 1, bool BUF = false>
__global__ __launch_bounds__(THREADS) void conv_wgrad_kernel(
    const float* __restrict__ dY, const float* __restrict__ X, float* __restrict__ out, float* __restrict__ dbias,
    WgradShape g, int want_bias, int accumulate)
{
    constexpr int TM = BM / 2, TN = BN / 2, FM = TM / 32, FN = TN / 32;
    // BKW = pixels per K step (16; 32 for the staged-split arithmetic, whose MFMA burst per step is 2.7x shorter)
    constexpr int A_PITCH = KStridedTile<BM, BKW>::PITCH, B_PITCH = KStridedTile<BN, BKW>::PITCH;
    constexpr int A_FLOATS = KStridedTile<BM, BKW>::FLOATS, B_FLOATS = KStridedTile<BN, BKW>::FLOATS;
    constexpr int A_LOADS = BKW * BM / 4 / THREADS, B_LOADS = BKW * BN / 4 / THREADS;      // float4 loads per thread and K step
    constexpr bool S3 = MMA == 3;                            // bf16 planes (igemm.h), both operands K-strided: transposed reads
    typedef KStridedPlanes<BM, BKW> AP3;
    typedef KStridedPlanes<BN, BKW> BP3;
    constexpr int LDS_BYTES = S3 ? 2 * (AP3::BYTES + BP3::BYTES) : 2 * (A_FLOATS + B_FLOATS) * 4;
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES];
    float* lds = reinterpret_cast<float*>(lds_raw);
    float* As = lds;
    float* Bs = lds + 2 * A_FLOATS;
    unsigned char* A3 = lds_raw;
    unsigned char* B3 = lds_raw + 2 * AP3::BYTES;

    const int NC = g.R * g.S * g.Ci;                         // GEMM N
    const int P = g.N * g.Ho * g.Wo;                         // GEMM K (pixels)
    const int tiles_n = (NC + BN - 1) / BN;
    const unsigned tile = xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (int)(tile / tiles_n) * BM, n0 = (int)(tile % tiles_n) * BN;
    const int p_begin = blockIdx.z * g.pix_per_split, p_end = min(P, p_begin + g.pix_per_split);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * TM, wn = (wave & 1) * TN;

    // column (r,q,c) of each B chunk this thread stages is fixed over the K loop
    int b_kk[B_LOADS], b_col[B_LOADS], b_r[B_LOADS], b_q[B_LOADS], b_c[B_LOADS];
    bool b_ok[B_LOADS];
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i) {
        const int idx = tid + THREADS * i;
        b_kk[i] = idx / (BN / 4);
        b_col[i] = (idx - b_kk[i] * (BN / 4)) * 4;
        const int col = n0 + b_col[i];
        b_ok[i] = col < NC;
        const int rs = b_ok[i] ? col / g.Ci : 0;
        b_c[i] = col - rs * g.Ci;
        b_r[i] = rs / g.S;
        b_q[i] = rs - b_r[i] * g.S;
    }

    // running (image, row, col) decomposition of the pixel each B chunk reads: divisions once, then carries
    int b_n[B_LOADS], b_oy[B_LOADS], b_ox[B_LOADS];
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i) {
        const int pp = min(p_begin + b_kk[i], max(P - 1, 0));
        b_n[i] = pp / (g.Ho * g.Wo);
        const int rem = pp - b_n[i] * (g.Ho * g.Wo);
        b_oy[i] = rem / g.Wo;
        b_ox[i] = rem - b_oy[i] * g.Wo;
    }
    int a_kk[A_LOADS], a_ch[A_LOADS];
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i) {
        const int idx = tid + THREADS * i;
        a_kk[i] = idx / (BM / 4);
        a_ch[i] = (idx - a_kk[i] * (BM / 4)) * 4;
    }

    f32x4 a_set[PF][A_LOADS], b_set[PF][B_LOADS], bsum[A_LOADS];
    unsigned m_set[PF];
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i) bsum[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    // ---- BUF: 32-bit byte offsets, out-of-range elements pushed past the end of the tensor (the hardware returns zeros) ----
    constexpr unsigned OOB = 0x80000000u;
    __amdgpu_buffer_rsrc_t y_rsrc, x_rsrc;
    int a_off[BUF ? A_LOADS : 1];
    float inv_wo = 0.f, inv_ho = 0.f;
    if constexpr (BUF) {
        y_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)dY, 0, (int)min((long)P * g.Co * 4, (long)0x7fffffff), 0x00020000);
        x_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)X, 0, (int)min((long)g.N * g.Hi * g.Wi * g.Ci * 4, (long)0x7fffffff), 0x00020000);
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) a_off[i] = m0 + a_ch[i] < g.Co ? (a_kk[i] * g.Co + m0 + a_ch[i]) * 4 : (int)OOB;
        inv_wo = 1.0f / (float)g.Wo; inv_ho = 1.0f / (float)g.Ho;
    }
    const bool bias_block = want_bias && n0 == 0;            // the first column tile also sums dY over the pixels
    // loads the K step that starts at pixel pt; MUST be called with pt = p_begin, p_begin+BK, ... in order
    // branch-free loads (masked chunks read element 0 and are zeroed on the LDS write): straight-line code, exact s_waitcnt
    auto load_global = [&](int pt, bool advance, f32x4 (&a_reg)[A_LOADS], f32x4 (&b_reg)[B_LOADS], unsigned& lmask) {
        lmask = 0;
        if (advance) {                                   // pixel carry of the B gather: BEFORE the loads, so that nothing but
#pragma unroll                                           // straight-line code sits between them and the MFMAs
            for (int i = 0; i < B_LOADS; ++i) {
                if constexpr (BUF) {
                    // branch-free (a branch costs the ring an s_waitcnt vmcnt(0)): wraps = floor(ox / Wo) by a float reciprocal
                    // (exact after one correction step for ox < 2^22), then the same for the rows
                    int ox = b_ox[i] + BKW;
                    int w = (int)((float)ox * inv_wo);
                    ox -= w * g.Wo;
                    const int lo = ox < 0, hi = ox >= g.Wo;
                    ox += lo ? g.Wo : 0; ox -= hi ? g.Wo : 0; w += hi - lo;
                    int oy = b_oy[i] + w;
                    int v = (int)((float)oy * inv_ho);
                    oy -= v * g.Ho;
                    const int lo2 = oy < 0, hi2 = oy >= g.Ho;
                    oy += lo2 ? g.Ho : 0; oy -= hi2 ? g.Ho : 0; v += hi2 - lo2;
                    b_ox[i] = ox; b_oy[i] = oy; b_n[i] += v;
                } else {
                    b_ox[i] += BKW;
                    while (b_ox[i] >= g.Wo) {
                        b_ox[i] -= g.Wo;
                        if (++b_oy[i] == g.Ho) { b_oy[i] = 0; ++b_n[i]; }
                    }
                }
            }
        }
        if constexpr (BUF) {
            const int s_a = pt * g.Co * 4;
#pragma unroll
            for (int i = 0; i < A_LOADS; ++i) {
                const bool ok = pt + a_kk[i] < p_end;
                a_reg[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(y_rsrc, ok ? a_off[i] + s_a : (int)OOB, 0, 0));
            }
#pragma unroll
            for (int i = 0; i < B_LOADS; ++i) {
                const int iy = b_oy[i] * g.stride - g.pad + b_r[i], ix = b_ox[i] * g.stride - g.pad + b_q[i];
                const bool ok = b_ok[i] && pt + b_kk[i] < p_end && (unsigned)iy < (unsigned)g.Hi && (unsigned)ix < (unsigned)g.Wi;
                const int off = (((b_n[i] * g.Hi + iy) * g.Wi + ix) * g.Ci + b_c[i]) * 4;
                b_reg[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, ok ? off : (int)OOB, 0, 0));
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) {
            const int p = pt + a_kk[i], co = m0 + a_ch[i];
            const bool ok = p < p_end && co < g.Co;
            a_reg[i] = *reinterpret_cast<const f32x4*>(dY + (ok ? (size_t)p * g.Co + co : 0));
            lmask |= (unsigned)ok << i;
        }
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i) {
            const int p = pt + b_kk[i];
            const int iy = b_oy[i] * g.stride - g.pad + b_r[i], ix = b_ox[i] * g.stride - g.pad + b_q[i];
            const bool ok = b_ok[i] && p < p_end && iy >= 0 && iy < g.Hi && ix >= 0 && ix < g.Wi;
            const int pix = ok ? (b_n[i] * g.Hi + iy) * g.Wi + ix : 0;
            b_reg[i] = *reinterpret_cast<const f32x4*>(X + (size_t)pix * g.Ci + (ok ? b_c[i] : 0));
            lmask |= (unsigned)ok << (16 + i);
        }
    };
    auto store_lds = [&](int buf, const f32x4 (&a_reg)[A_LOADS], const f32x4 (&b_reg)[B_LOADS], unsigned lmask) {
        const f32x4 zero{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) {
            const f32x4 v = BUF ? a_reg[i] : ((lmask >> i) & 1u ? a_reg[i] : zero);
            if (bias_block) bsum[i] += v;
            if (S3) store_split3<AP3::PLANE>(A3 + buf * AP3::BYTES, a_kk[i] * AP3::PITCH + a_ch[i] * 2, v);
            else *reinterpret_cast<f32x4*>(As + buf * A_FLOATS + a_kk[i] * A_PITCH + a_ch[i]) = v;
        }
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i) {
            const f32x4 v = BUF ? b_reg[i] : ((lmask >> (16 + i)) & 1u ? b_reg[i] : zero);
            if (S3) store_split3<BP3::PLANE>(B3 + buf * BP3::BYTES, b_kk[i] * BP3::PITCH + b_col[i] * 2, v);
            else *reinterpret_cast<f32x4*>(Bs + buf * B_FLOATS + b_kk[i] * B_PITCH + b_col[i]) = v;
        }
    };

    // unsplit + accumulate: start the accumulators from the old gradient (its HBM latency overlaps the first tile's loads;
    // the epilogue is then a plain store instead of a read-modify-write)
    const bool from_old = g.splits == 1 && accumulate;
    f32x16 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int n = n0 + wn + j * 32 + frag_col(lane), m = m0 + wm + i * 32 + frag_row(lane, e);
                const bool ok = from_old && n < NC && m < g.Co;
                const float v = out[ok ? (size_t)m * NC + n : 0];                 // branch-free: all 16 reads in flight together
                acc[i][j][e] = ok ? v : 0.f;
            }

    if (p_begin < p_end) {
        const int nsteps = (p_end - p_begin + BKW - 1) / BKW;
#pragma unroll
        for (int d = 0; d < PF; ++d) load_global(p_begin + d * BKW, d > 0, a_set[d], b_set[d], m_set[d]);
        store_lds(0, a_set[0], b_set[0], m_set[0]);
        __syncthreads();
        int buf = 0;
        auto iteration = [&](auto U, int tt) {
            constexpr int u = decltype(U)::value;
            load_global(p_begin + (tt + PF) * BKW, true, a_set[u], b_set[u], m_set[u]);       // past the end: fully masked
#pragma unroll
            for (int ks = 0; ks < BKW / BK; ++ks) {
                if (S3) {
                    Frag3 a[FM], b[FN];
                    read_kstrided3<FM, AP3::PITCH, AP3::PLANE>(A3 + buf * AP3::BYTES + wm * 2, lane, ks, a);
                    read_kstrided3<FN, BP3::PITCH, BP3::PLANE>(B3 + buf * BP3::BYTES + wn * 2, lane, ks, b);
                    mma3_step<FM, FN>(a, b, acc);
                } else {
                    float a[FM][8], b[FN][8];
                    read_kstrided<FM, A_PITCH>(As + buf * A_FLOATS + wm, lane, ks, a);
                    read_kstrided<FN, B_PITCH>(Bs + buf * B_FLOATS + wn, lane, ks, b);
                    mma_any<S3 ? 0 : MMA, FM, FN>(a, b, acc);
                }
            }
            if (PF == 1) __builtin_amdgcn_sched_barrier(0);           // the LDS fill (and its wait for the loads) stays behind the MFMAs
            constexpr int v = (u + 1) % PF;
            store_lds(buf ^ 1, a_set[v], b_set[v], m_set[v]);
            if (PF > 1 && S3 && g_interleave) {
#pragma unroll
                for (int i = 0; i < 6 * FM * FN * (BKW / BK); ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, (14 + FM * FN - 1) / (FM * FN), 0);
                }
            }
            __syncthreads();
            buf ^= 1;
        };
        int t = 0;
        for (; t + PF <= nsteps; t += PF) unroll_iterations<PF>(iteration, t);
        if (PF > 1) tail_iterations<PF - 1>(iteration, t, nsteps);
    }
    const bool direct = g.splits == 1;
    float* dst = direct ? out : out + (size_t)blockIdx.z * ((size_t)g.Co * NC + g.Co);
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int n = n0 + wn + j * 32 + frag_col(lane);
        if (n >= NC) continue;
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wm + i * 32 + frag_row(lane, e);
                if (m < g.Co) {
                    float* q = dst + (size_t)m * NC + n;
                    *q = acc[i][j][e];
                }
            }
    }
    if (bias_block) {
        // per-thread sums cover rows a_kk of every K step; fold the BK rows through LDS (reusing the A image)
        __syncthreads();
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i)
            *reinterpret_cast<f32x4*>(As + a_kk[i] * A_PITCH + a_ch[i]) = bsum[i];
        __syncthreads();
        if (tid < BM && m0 + tid < g.Co) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < BKW; ++k) t += As[k * A_PITCH + tid];
            if (direct) dbias[m0 + tid] = accumulate ? dbias[m0 + tid] + t : t;
            else dst[(size_t)g.Co * NC + m0 + tid] = t;
        }
    }
}

// ---- weight gradient of a 3x3 / stride 1 / pad 1 convolution: the three taps of a filter row from ONE staged pixel block ----
// The generic kernel above treats the 9 taps as 9 column tiles: every (co tile, tap, ci tile) workgroup loads, splits and
// stages its own dY block and its own (shifted) X block.  The taps (dy, -1), (dy, 0), (dy, +1) read the SAME 16 dY pixels and
// X rows that differ by one pixel, so here one workgroup of 12 waves stages dY[16 px][64 co] and X[18 px][64 ci] once per K
// step and three groups of 4 waves multiply them - group dx reads the X planes one row further down and, where a pixel of
// the block sits on the image border its tap would cross (x = 0 for dx = -1, x = W-1 for dx = +1: at most one pixel per 16,
// W >= 16), clears that pixel's element of its dY fragment.  Loads, split arithmetic and LDS fills per MFMA fall 2.8x; the
// output tile (3 x 64x64) and the partial-sum traffic per MFMA stay what they were.  X rows whose image row y + dy falls
// outside the frame are staged as zeros (the pixel block may span image rows and frames: rows are tested one by one).
// bf16x3 arithmetic, buffer loads; Ci, Co multiples of 64.
constexpr int W3_THREADS = 768;
template <int BKW> struct Wgrad3Lds : Wgrad3Image<BKW> {
    static constexpr int BYTES = 6 * Wgrad3Image<BKW>::IMG + 2 * Wgrad3Image<BKW>::PLANE + 512;      // 3 buffers x 2 operands + a dump area for the idle staging lanes
};
template <int PF, int BKW>
__global__ __launch_bounds__(W3_THREADS) void conv_wgrad3x3_kernel(
    const float* __restrict__ dY, const float* __restrict__ X, float* __restrict__ out, float* __restrict__ dbias,
    WgradShape g, int want_bias, int accumulate)
{
    constexpr int NSUB = BKW / BK;                           // 16-pixel MFMA sub-steps per K step
    typedef Wgrad3Lds<BKW> L;
    constexpr int PITCH = L::PITCH, PLANE = L::PLANE, IMG = L::IMG;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];               // [buf 0..2][dY | X][plane][row][col], dump
    static_assert(PF % 2 == 0 && (NSUB == 1 || NSUB == 2), "fragment parity is read off the ring slot");

    const int NC = 9 * g.Ci, W = g.Wi, H = g.Hi;
    const int P = g.N * H * W;
    const Wgrad3Tile t3 = wgrad3_tile(blockIdx.x, gridDim.x, g.Ci);
    const int m0 = t3.m0, c0 = t3.c0, dy = t3.dy;
    const int p_begin = blockIdx.z * g.pix_per_split, p_end = min(P, p_begin + g.pix_per_split);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Wgrad3Wave w3 = wgrad3_wave(wave);
    const int dx = w3.dx, wm = w3.wm, wn = w3.wn;

    // ---- staging roles (wave-uniform): waves 0-3 dY, waves 4-7 X rows 0..BKW-1 (row kk + 16 i each), wave 8 (first half) the
    // two X rows BKW, BKW+1 ----
    const bool role_a = wave < 4, halo = wave == 8;
    const int st = tid - (role_a ? 0 : (halo ? 512 : 256));
    const int kk = (st >> 4) + (halo ? BKW : 0), col = (st & 15) * 4;                     // first row of the image, first of 4 columns
    const float* src = role_a ? dY : X;
    const int cs = role_a ? g.Co : g.Ci;                     // channels of the source tensor
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, (int)min((long)P * cs * 4, (long)0x7fffffff), 0x00020000);
    constexpr unsigned OOB = 0x80000000u;
    bool active[NSUB];
    int off_c[NSUB], t_cur[NSUB], t_x[NSUB], t_y[NSUB], st_off[NSUB];
#pragma unroll
    for (int i = 0; i < NSUB; ++i) {
        const int row = kk + 16 * i;
        active[i] = wave < 8 || (halo && lane < 32 && i == 0);
        // dY: element (pt + row, m0 + col); X: aligned pixel t = pt - 1 + row, source pixel t + dy * W, channel c0 + col
        off_c[i] = role_a ? (row * cs + m0 + col) * 4 : ((row - 1 + dy * W) * cs + c0 + col) * 4;
        t_cur[i] = p_begin + row - (role_a ? 0 : 1);         // dY: the pixel; X: the aligned pixel
        const int tt = t_cur[i] + W * H;                     // >= 0; same (x, y) as t_cur
        const int rowi = tt / W;
        t_x[i] = tt - rowi * W;
        t_y[i] = rowi % H;
        // lanes without a staging job write their (zero) chunk into the dump area behind the images: the loop body stays one
        // basic block, so that the scheduler can interleave the split with the MFMAs
        st_off[i] = active[i] ? (role_a ? 0 : IMG) + row * PITCH + col * 2 : 6 * IMG + lane * 8;
    }
    f32x4 set[PF][NSUB];
    f32x4 bsum = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool bias_block = want_bias && t3.ct == 0 && t3.dyi == 0;
    const float bflag = (role_a && bias_block) ? 1.f : 0.f;
    // loads the K step that starts at pixel pt; MUST be called with pt = p_begin, p_begin + BKW, ... in order (branch-free)
    auto load_global = [&](int pt, f32x4 (&reg)[NSUB]) {
#pragma unroll
        for (int i = 0; i < NSUB; ++i) {
            const bool ok_a = t_cur[i] < p_end;
            const bool ok_b = (unsigned)t_cur[i] < (unsigned)P && (unsigned)(t_y[i] + dy) < (unsigned)H;
            const bool ok = active[i] && (role_a ? ok_a : ok_b);
            reg[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, ok ? off_c[i] + pt * cs * 4 : (int)OOB, 0, 0));
            t_cur[i] += BKW;
            t_x[i] += BKW;
#pragma unroll
            for (int r = 0; r < NSUB; ++r) {                 // W >= 16: at most NSUB row wraps per step
                const int wx = t_x[i] >= W;
                t_x[i] -= wx ? W : 0;
                t_y[i] += wx;
                t_y[i] = t_y[i] == H ? 0 : t_y[i];
            }
        }
    };
    auto store_lds = [&](int buf_off, const f32x4 (&v)[NSUB]) {
#pragma unroll
        for (int i = 0; i < NSUB; ++i) {
            bsum += v[i] * bflag;
            store_split3<PLANE>(lds_raw, st_off[i] + (active[i] ? buf_off : 0), v[i]);
        }
    };

    const bool from_old = g.splits == 1 && accumulate;
    const int n_base = wgrad3_n_base(t3, w3, g.Ci);
    f32x16 acc[1][1];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[0][0][e] = wgrad3_acc_start(out, from_old, m0 + wm, n_base, NC, lane, e);

    if (p_begin < p_end) {
        // Software pipeline over the 16-pixel sub-steps (all 12 waves of the CU's one workgroup run in lock-step, so nothing
        // else hides an LDS round trip): while sub-step s is multiplied, the fragments of sub-step s+1 - the next one of this
        // K step, or the first one of the next K step - travel from LDS into the other register set.  Three LDS buffers: in
        // iteration t step t is read, step t+1 is read (its first sub-step) and step t+2 is written (into the buffer step t-1
        // left before the last barrier); the ring slot it came from takes step t+2+PF.  One barrier per K step.
        const int nsteps = (p_end - p_begin + BKW - 1) / BKW;
        int mx = p_begin % W;                                // image column of the first pixel of the sub-step whose fragment is masked next
#pragma unroll
        for (int d = 0; d < PF; ++d) load_global(p_begin + d * BKW, set[d]);
        store_lds(0, set[0]);
        load_global(p_begin + PF * BKW, set[0]);
        store_lds(2 * IMG, set[1 % PF]);
        load_global(p_begin + (PF + 1) * BKW, set[1 % PF]);
        __syncthreads();
        Frag3 fa[2], fb[2];
        const unsigned char* a_src = lds_raw + wm * 2;
        const unsigned char* b_src = lds_raw + IMG + (dx + 1) * PITCH + wn * 2;
        auto read_frags = [&](int buf_off, int ks, Frag3& a, Frag3& b) {
            wgrad3_read_frags<PITCH, PLANE>(a_src + buf_off, b_src + buf_off, lane, ks, a, b);
        };
        const int h8 = (lane >> 5) * 8;
        read_frags(0, 0, fa[0], fb[0]);
        int o_cur = 0, o_nxt = 2 * IMG, o_st = 4 * IMG;       // byte offsets of the buffers of steps t, t+1, t+2
        auto iteration = [&](auto U, int tt) {
            constexpr int u = decltype(U)::value;             // tt % PF
            constexpr int slot = (u + 2) % PF;
#pragma unroll
            for (int ks = 0; ks < NSUB; ++ks) {
                const int cur = (u * NSUB + ks) & 1, nxt = cur ^ 1;
                {
                    const int ke = dx < 0 ? (mx == 0 ? 0 : W - mx) : W - 1 - mx;              // mask, then read: the order wgrad3s.hip turns round
                    if (dx != 0 && ke < BK) wgrad3_mask_edge(fa[cur], ke, h8);
                    mx += BK;
                    mx -= mx >= W ? W : 0;
                }
                if (ks + 1 < NSUB) read_frags(o_cur, ks + 1, fa[nxt], fb[nxt]);
                else read_frags(o_nxt, 0, fa[nxt], fb[nxt]);
                Frag3 (&a)[1] = *reinterpret_cast<Frag3 (*)[1]>(&fa[cur]);
                Frag3 (&b)[1] = *reinterpret_cast<Frag3 (*)[1]>(&fb[cur]);
                mma3_step<1, 1>(a, b, acc);
            }
            store_lds(o_st, set[slot]);                       // step tt + 2
            load_global(p_begin + (tt + 2 + PF) * BKW, set[slot]);                        // past the end: fully masked
#pragma unroll
            for (int i = 0; i < 6; ++i) {                     // an MFMA, then a few of the split / address instructions, ...
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
            }
            __syncthreads();
            const int o = o_cur; o_cur = o_nxt; o_nxt = o_st; o_st = o;
        };
        int t = 0;
        for (; t + PF <= nsteps; t += PF) unroll_iterations<PF>(iteration, t);
        if (PF > 1) tail_iterations<PF - 1>(iteration, t, nsteps);
    }
    const bool direct = g.splits == 1;
    float* dst = wgrad3_store(out, g.splits, blockIdx.z, g.Co, NC, m0 + wm, n_base, lane, acc[0][0]);
    if (bias_block) {
        // the dY staging threads hold the sums of rows kk + 16 i of every step: fold the 16 row classes through LDS
        float* fold = reinterpret_cast<float*>(lds_raw);
        __syncthreads();
        if (role_a) *reinterpret_cast<f32x4*>(fold + kk * 68 + col) = bsum;
        __syncthreads();
        if (tid < 64) {
            float tsum = 0.f;
#pragma unroll
            for (int k = 0; k < BK; ++k) tsum += fold[k * 68 + tid];
            if (direct) dbias[m0 + tid] = accumulate ? dbias[m0 + tid] + tsum : tsum;
            else dst[(size_t)g.Co * NC + m0 + tid] = tsum;
        }
    }
}

template <int BM, int BN, int MMA = 0>
__global__ __launch_bounds__(THREADS) void linear_wgrad_smallp_kernel(
    const float* __restrict__ dY, const float* __restrict__ X, float* __restrict__ dw, float* __restrict__ dbias,
    int P, int Co, int Ci, int want_bias, int accumulate)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    smallp_tile<BM, BN, false, MMA>(dY, X, dw, dbias, P, Co, Ci, want_bias, accumulate, lds, blockIdx.x, gridDim.x);
}

// dW (+)= sum_z part[z][0:nw],  dbias (+)= sum_z part[z][nw:nw+nb]   (part rows are nw+nb floats long; nw, nb multiples of 4)
// 256 threads = 64 float4 columns x 4 split groups: group g sums the partials z = g, g+4, ... with four loads in flight, the
// four group sums are folded through LDS in a fixed order (deterministic).  The small trunk layers run with 40-190 splits;
// one thread per element walking all of them paid one L2 latency per split (22-62 us per launch, now a few).
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                           float* __restrict__ dbias, long nw, long nb, int splits, int accumulate)
{
    __shared__ f32x4 red[3][64];
    const int lane = threadIdx.x & 63, zg = threadIdx.x >> 6;
    const long total4 = (nw + nb) >> 2;
    const long i4 = (long)blockIdx.x * 64 + lane;
    const bool ok = i4 < total4;
    const long i = i4 * 4;
    const bool is_w = i < nw;
    const bool writer = zg == 0 && ok && (is_w || dbias);
    const f32x4 zero{0.f, 0.f, 0.f, 0.f};
    f32x4 old = zero;
    if (writer && accumulate) {                           // cold read first: it overlaps the partial sums
        if (is_w) old = *reinterpret_cast<const f32x4*>(dw + i);
        else { const float* b = dbias + (i - nw); old = f32x4{b[0], b[1], b[2], b[3]}; }
    }
    const f32x4* p = reinterpret_cast<const f32x4*>(part) + (ok ? i4 : 0);
    f32x4 s = zero;
    int z = zg;
    for (; z + 12 < splits; z += 16) {
        const f32x4 v0 = p[(long)z * total4], v1 = p[(long)(z + 4) * total4], v2 = p[(long)(z + 8) * total4],
                    v3 = p[(long)(z + 12) * total4];
        s += v0; s += v1; s += v2; s += v3;
    }
    for (; z < splits; z += 4) s += p[(long)z * total4];
    if (zg) red[zg - 1][lane] = s;
    __syncthreads();
    if (writer) {
        const f32x4 t = old + ((s + red[0][lane]) + (red[1][lane] + red[2][lane]));
        if (is_w) *reinterpret_cast<f32x4*>(dw + i) = t;
        else { float* b = dbias + (i - nw); b[0] = t.x; b[1] = t.y; b[2] = t.z; b[3] = t.w; }
    }
}

}  // namespace

// Weight gradient.  dw OHWI [Co][R][S][Ci] is overwritten (accumulate=0) or added to (accumulate=1).
// workspace must hold splits*Co*R*S*Ci floats; query with phnet_conv2d_wgrad_workspace.
static long wgrad_splits(long P, long Co, long NC, int* bm_out)
{
    // measured (bench_conv.py --trunk --wgrad, reduce included): on a 5-frame clip 128-row tiles win at Co = 128 only (73 vs 79 us);
    // at Co = 256 / 512 (5000 / 1250 pixels) the 64x64 tile with more splits is 5 / 3 us faster; with 8 clips per step
    // (40000 / 10000 pixels) the 128-row tile wins everywhere (step 129.7 vs 132.4 ms)
    const int bm = (Co >= 128 && (Co < 256 || P > 8192) && tuning().wgrad_bm128) ? 128 : 64;
    const long tiles = ceil_div64(Co, bm) * ceil_div64(NC, 64);
    const long target = tiles >= 64 ? max((long)tuning().wgrad_target, (long)1250) : (long)tuning().wgrad_target;   // measured: bench_conv --wgrad
    long splits = max((long)1, min((long)256, target / max((long)1, tiles)));
    splits = max((long)1, min(splits, P / 64));
    // the M=240 linears of the lane head (15 K steps in all): with >= 32 tiles a split only adds a reduce launch;
    // unsplit launches also accumulate straight into the gradient arena
    if (P <= 1024 && tiles >= 32) splits = 1;
    if (bm_out) *bm_out = bm;
    return splits;
}

// the three-taps kernel (conv_wgrad3x3_kernel): 3x3 / stride 1 / pad 1, channel counts in whole 64-tiles, bf16x3 arithmetic
static bool wgrad3_applies(long P, int Hi, int Wi, int Ci, int Co, int R, int S, int stride, int pad)
{
    return tuning().wgrad3 && tuning().mma_mode == 3 && R == 3 && S == 3 && stride == 1 && pad == 1 && (Ci & 63) == 0 && (Co & 63) == 0 &&
           Wi >= BK && P >= 64 && P * (long)max(Ci, Co) * 4 < 0x7fffffffL;
}
static long wgrad3_splits(long P, long Co, long Ci)
{
    const long tiles = (Co / 64) * (Ci / 64) * 3;
    return max((long)1, min(min((long)256, P / 64), (tuning().wgrad3_target + tiles / 2) / tiles));
}

PHNET_API uint64_t phnet_conv2d_wgrad_workspace(int32_t N, int32_t Hi, int32_t Wi, int32_t Ci, int32_t Co,
                                                int32_t R, int32_t S, int32_t stride, int32_t pad)
{
    const long Ho = (Hi + 2 * pad - R) / stride + 1, Wo = (Wi + 2 * pad - S) / stride + 1;
    const long P = (long)N * Ho * Wo, NC = (long)R * S * Ci;
    long splits = wgrad_splits(P, Co, NC, nullptr);
    if (R == 3 && S == 3 && stride == 1 && pad == 1 && (Ci & 63) == 0 && (Co & 63) == 0)     // whichever kernel the call picks
        splits = max(splits, min(min((long)256, max((long)1, P / 64)), (long)(1024 / ((Co / 64) * (Ci / 64) * 3) + 1)));
    return (uint64_t)(splits * (Co * NC + Co) * sizeof(float));
}

// What one weight-gradient call launches.  Decided once (pick_wgrad); phnet_conv2d_wgrad launches it, wgrad_kernel_name spells it.
enum class WgradFamily { SmallP, ThreeTapsPC, ThreeTaps, ManyRowsPC, Generic };     // linear_wgrad_smallp | wgrad3s | conv_wgrad3x3 | wgrad1s | conv_wgrad
struct WgradPick {
    WgradFamily family;
    int bm, bkw, mma;                    // output rows per tile; pixels per K step (0: the whole range at once); arithmetic
    long splits;
};


static WgradPick pick_wgrad(const WgradShape& g, bool has_dbias, bool has_ws, uint64_t ws_bytes)
{
    const Tuning& tn = tuning();
    const int Ci = g.Ci, Co = g.Co;
    const long P = (long)g.N * g.Ho * g.Wo, NC = (long)g.R * g.S * Ci;
    const bool linear = g.R == 1 && g.S == 1 && g.stride == 1 && g.pad == 0;
    auto fit = [&](long splits) {                                        // the split factor whose partial sums the workspace holds
        const long row = (long)Co * NC + Co;
        while (splits > 1 && (!has_ws || (uint64_t)(splits * row * sizeof(float)) > ws_bytes)) --splits;
        return splits;
    };
    // Linear over few rows with up to a few hundred output tiles (with thousands of tiles the generic kernel keeps several
    // workgroups per CU in flight, which hides the same latency; this one needs 139 KB of LDS = one workgroup per CU)
    if (linear && P <= SMALLP_MAX && tn.wgrad_smallp && ceil_div64(Co, 64) * ceil_div64(Ci, 64) < tn.smallp_max_tiles)
        return {WgradFamily::SmallP, 64, 0, tn.mma_mode == 1 ? 1 : 0, 1};
    if (wgrad3_applies(P, g.Hi, g.Wi, Ci, Co, g.R, g.S, g.stride, g.pad)) {
        const long splits = fit(wgrad3_splits(P, Co, Ci));
        // producer / consumer kernel: no bias gradient, and an image holds >= one K step
        if (tn.wgrad3s && !has_dbias && (long)g.Hi * g.Wi >= phnet_wgrad3s_kstep()) return {WgradFamily::ThreeTapsPC, 64, phnet_wgrad3s_kstep(), 3, splits};
        return {WgradFamily::ThreeTaps, 64, tn.wgrad3_bkw == 16 ? 16 : 32, 3, splits};
    }
    // Linear / 1x1 layers over many rows with >= 64 tiles of 128 x 128: the producer / consumer kernel (csrc/wgrad1s.hip)
    if (tn.wgrad1s && tn.mma_mode == 3 && linear && (Co & 127) == 0 && (Ci & 127) == 0 && P >= 256 &&
        (long)(Co / 128) * (Ci / 128) >= 64 && P * (long)max(Ci, Co) * 4 < 0x7fffffffL) {
        // at most 256 / 64 = 4 splits of >= 128 rows = 8 steps each: steps >= 8 * splits > splits * (splits - 1), so the last
        // split can be short but never empty.  (The other families can get an empty one - 391 pixels, 6 splits: 25 steps of 16
        // in splits of 5 - and their kernels then write zeros: tests/gemm_cases.py "empty_split".)
        const long tiles = (long)(Co / 128) * (Ci / 128);
        return {WgradFamily::ManyRowsPC, 128, phnet_wgrad1s_kstep(), 3, fit(max((long)1, min((long)(P / 128), (long)256 / tiles)))};
    }
    int bm = 64;
    const long splits = fit(wgrad_splits(P, Co, NC, &bm));
    return {WgradFamily::Generic, bm, (tn.mma_mode == 3 && tn.wgrad_bkw == 32) ? 32 : BK, tn.mma_mode, splits};
}

// the instantiation the switch of phnet_conv2d_wgrad below launches for a pick, as rocprofv3 spells it
static int wgrad_kernel_name(const WgradPick& p, char* name, int cap)
{
    int n;
    switch (p.family) {
    case WgradFamily::SmallP: n = snprintf(name, (size_t)cap, "linear_wgrad_smallp_kernel<64, 64, %d>", p.mma); break;
    case WgradFamily::ThreeTapsPC: n = snprintf(name, (size_t)cap, "wgrad3s_kernel<%d>", p.bkw / BK); break;
    case WgradFamily::ThreeTaps: n = snprintf(name, (size_t)cap, "conv_wgrad3x3_kernel<4, %d>", p.bkw); break;
    case WgradFamily::ManyRowsPC: n = snprintf(name, (size_t)cap, "wgrad1s_kernel"); break;
    default: n = snprintf(name, (size_t)cap, "conv_wgrad_kernel<%d, 64, %d, %d, %d, %s>", p.bm, p.mma, p.bkw,
                          p.mma == 3 ? (p.bkw == 32 ? 2 : 4) : 1, p.mma == 3 ? "true" : "false");
    }
    return n < cap ? PHNET_OK : PHNET_ERR_ARG;
}

// Host-only query: the kernel instantiation phnet_conv2d_wgrad launches for the same shape arguments, and its split factor.
PHNET_API int phnet_conv2d_wgrad_kernel(int32_t N, int32_t Hi, int32_t Wi, int32_t Ci, int32_t Co, int32_t R, int32_t S, int32_t stride,
                                        int32_t pad, int32_t has_dbias, uint64_t ws_bytes, char* name, int32_t name_cap, int32_t* splits)
{
    WgradShape g;
    if (!wgrad_shape(N, Hi, Wi, Ci, Co, R, S, stride, pad, &g) || !name || name_cap < 1 || !splits) return PHNET_ERR_ARG;
    if (tuning().mma_mode == 4) return PHNET_ERR_ARG;               // the bf16 inference arithmetic is forward-only
    const WgradPick p = pick_wgrad(g, has_dbias != 0, ws_bytes > 0, ws_bytes);
    *splits = (int32_t)p.splits;
    return wgrad_kernel_name(p, name, name_cap);
}

// dw OHWI [Co][R][S][Ci] and (optionally) dbias [Co] = sum of dy over all pixels are overwritten (accumulate=0) or
// added to (accumulate=1).  workspace: phnet_conv2d_wgrad_workspace bytes (split-K partial sums; unused when the
// problem runs unsplit).
PHNET_API int phnet_conv2d_wgrad(const float* dy, const float* x, float* dw, float* dbias,
                                 int32_t N, int32_t Hi, int32_t Wi, int32_t Ci, int32_t Co, int32_t R, int32_t S,
                                 int32_t stride, int32_t pad, int32_t accumulate,
                                 void* workspace, uint64_t ws_bytes, void* stream)
{
    WgradShape g;
    if (!wgrad_shape(N, Hi, Wi, Ci, Co, R, S, stride, pad, &g) || !dy || !x || !dw) return PHNET_ERR_ARG;
    if (tuning().mma_mode == 4) return PHNET_ERR_ARG;               // the bf16 inference arithmetic is forward-only
    const WgradPick p = pick_wgrad(g, dbias != nullptr, workspace != nullptr, ws_bytes);
    const long P = (long)N * g.Ho * g.Wo, NC = (long)R * S * Ci;
    hipStream_t st = (hipStream_t)stream;
    const int want_bias = dbias != nullptr;
    float* out = p.splits > 1 ? (float*)workspace : dw;
    g.splits = (int)p.splits;
    if (p.bkw) g.pix_per_split = (int)(ceil_div64(ceil_div64(max(P, (long)1), p.bkw), p.splits) * p.bkw);
    switch (p.family) {
    case WgradFamily::SmallP: {
        const int P16 = ((int)P + 15) & ~15;
        const size_t lds = (size_t)P16 * (64 + 4) * 2 * sizeof(float);
        static bool attr = false;
        if (!attr && !(attr = phnet_allow_dynamic_lds({(const void*)linear_wgrad_smallp_kernel<64, 64, 0>, (const void*)linear_wgrad_smallp_kernel<64, 64, 1>},
                                                      (int)((size_t)SMALLP_MAX * 68 * 2 * sizeof(float)))))
            return PHNET_ERR_LAUNCH;
        const long tiles = ceil_div64(Co, 64) * ceil_div64(Ci, 64);
        if (p.mma == 1)
            hipLaunchKernelGGL((linear_wgrad_smallp_kernel<64, 64, 1>), dim3((unsigned)tiles), dim3(THREADS), lds, st, dy, x, dw, dbias,
                               (int)P, Co, Ci, want_bias, accumulate);
        else
            hipLaunchKernelGGL((linear_wgrad_smallp_kernel<64, 64, 0>), dim3((unsigned)tiles), dim3(THREADS), lds, st, dy, x, dw, dbias,
                               (int)P, Co, Ci, want_bias, accumulate);
        break;
    }
    case WgradFamily::ThreeTapsPC: {
        const int rc = phnet_wgrad3s_launch(dy, x, out, Wgrad3sShape{N, Hi, Wi, Ci, Co, g.splits, g.pix_per_split}, accumulate, st);
        if (rc != PHNET_OK) return rc;
        break;
    }
    case WgradFamily::ThreeTaps: {
        dim3 grid((unsigned)((Co / 64) * (Ci / 64) * 3), 1, (unsigned)p.splits);
        static bool attr = false;
        if (!attr && !(attr = phnet_allow_dynamic_lds({(const void*)conv_wgrad3x3_kernel<4, 16>}, Wgrad3Lds<16>::BYTES) &&
                              phnet_allow_dynamic_lds({(const void*)conv_wgrad3x3_kernel<4, 32>}, Wgrad3Lds<32>::BYTES)))
            return PHNET_ERR_LAUNCH;
        if (p.bkw == 16)
            hipLaunchKernelGGL((conv_wgrad3x3_kernel<4, 16>), grid, dim3(W3_THREADS), Wgrad3Lds<16>::BYTES, st, dy, x, out, dbias, g, want_bias, accumulate);
        else
            hipLaunchKernelGGL((conv_wgrad3x3_kernel<4, 32>), grid, dim3(W3_THREADS), Wgrad3Lds<32>::BYTES, st, dy, x, out, dbias, g, want_bias, accumulate);
        break;
    }
    case WgradFamily::ManyRowsPC: {
        const int rc = phnet_wgrad1s_launch(dy, x, out, dbias, Wgrad1sShape{(int)P, Ci, Co, g.splits, g.pix_per_split}, accumulate, st);
        if (rc != PHNET_OK) return rc;
        break;
    }
    case WgradFamily::Generic: {
        dim3 grid((unsigned)(ceil_div64(Co, p.bm) * ceil_div64(NC, 64)), 1, (unsigned)p.splits);
#define PHNET_LAUNCH_WGRAD(...)                                                                                         \
    hipLaunchKernelGGL((conv_wgrad_kernel<__VA_ARGS__>), grid, dim3(THREADS), 0, st, dy, x, out, dbias, g, want_bias, accumulate)
        if (p.mma == 3 && p.bkw == 32 && p.bm == 128) PHNET_LAUNCH_WGRAD(128, 64, 3, 32, 2, true);
        else if (p.mma == 3 && p.bkw == 32) PHNET_LAUNCH_WGRAD(64, 64, 3, 32, 2, true);
        else if (p.mma == 3 && p.bm == 128) PHNET_LAUNCH_WGRAD(128, 64, 3, 16, 4, true);
        else if (p.mma == 3) PHNET_LAUNCH_WGRAD(64, 64, 3, 16, 4, true);
        else if (p.bm == 128 && p.mma == 2) PHNET_LAUNCH_WGRAD(128, 64, 2);
        else if (p.mma == 2) PHNET_LAUNCH_WGRAD(64, 64, 2);
        else if (p.bm == 128 && p.mma == 1) PHNET_LAUNCH_WGRAD(128, 64, 1);
        else if (p.mma == 1) PHNET_LAUNCH_WGRAD(64, 64, 1);
        else if (p.bm == 128) PHNET_LAUNCH_WGRAD(128, 64);
        else PHNET_LAUNCH_WGRAD(64, 64);
#undef PHNET_LAUNCH_WGRAD
        break;
    }
    }
    if (p.splits > 1) {                                                  // the partial sums of every family share one layout
        const long nw = (long)Co * NC, nb = Co;
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)ceil_div64((nw + nb) >> 2, 64)), dim3(256), 0, st,
                           (const float*)workspace, dw, dbias, nw, nb, (int)p.splits, accumulate);
    }
    return phnet_launch_status();
}
