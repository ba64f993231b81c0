// Implicit-GEMM convolution / linear kernels on fp32 MFMA for gfx950 (NHWC activations, OHWI weights).
//
// Replaces, for the hot path of SURVEY.md 8(a): the cuDNN convolutions behind
//   libs/models/resnet.py:79-95,293-307 (trunk), libs/models/fpn.py:109-163 (neck)
// and the cuBLAS addmm behind every nn.Linear of the head (Router4OL.py:308-392,
// utils/dynamic_head.py:31-59, Router.py:72-81), forward and data-gradient (weight gradient: conv_wgrad.hip).
//
//   forward : out[m][co] = sum_{r,q,c} X[n, oy*s-p+r, ox*s-p+q, c] * W[co][r][q][c]      (+bias)(+relu)
//             GEMM  M = N*Ho*Wo pixels, N = Co, K = R*S*Ci;  A gathered on the fly (K-contiguous),
//             B = W as stored (K-contiguous).
//   dgrad   : dX[m][c] = sum_{r,q,co} dY[n, (y+p-r)/s, (x+p-q)/s, co] * W[co][r][q][c]
//             same kernel: A gathered from dY with "input dilation" s, B read K-strided straight out
//             of the OHWI weights (row (r,q,co) -> W[co][R-1-r'][S-1-q'][:]) - no weight transpose pass.
// A Linear layer is the R=S=1 case on an [M,1,1,K] image.
//
// Roofline of arithmetic mode 0 (f32-input MFMA): MFMA-bound, 157.3 TF/s dense.  Algorithmic FLOPs = 2*M*N*K.
#include <cstdio>
#include "conv_igemm.h"
#include "tuning.h"
#include "linrows.h"

using namespace igemm;

namespace {

// ---- 3x3 / stride 1 / pad 1 forward and data gradient: the three taps of a filter row from ONE staged pixel block ----------
// In the generic tile program every K step gathers its own A block: the steps of the taps (dy,-1), (dy,0), (dy,+1) fetch, split
// and stage the SAME pixels shifted by one.  Here a "unit" = (filter row dy, 16-channel chunk) stages the 66 pixels m0-1 ..
// m0+64 of the shifted image row ONCE (bf16 planes, K-contiguous) and runs three K steps on it: step dx reads its A fragments
// dx rows further down the image and only the 64x16 weight tile is staged per step.  A-side loads, split arithmetic and LDS
// fills fall 2.9x - a third of the loop's operand traffic and vector instructions.  Measured: -2..-4 % (forward) and -6 % (dgrad)
// per layer, step -0.19 ms: what remains is the loop skeleton (one barrier and one 6-MFMA burst per wave and step).
// Rows whose tap leaves the image row (x = 0 for dx = -1, x = W-1 for dx = +1) are zeroed in
// the fragment (a per-lane select, the flags are fixed over the K loop); block rows whose image row y + dy is outside the frame -
// the block may span image rows and frames - are staged as zeros.  64x64 tile, 4 waves, bf16x3 arithmetic, buffer loads,
// prefetch ring of one unit (three weight tiles + the next A block); epilogue (bias / addend / ReLU / BatchNorm statistics /
// split-K partials) as in igemm_tile.  DGRAD: the same gather on dY with the flipped, transposed weight as B (K-strided planes).
constexpr int T3_AROWS = 66;
template <bool DGRAD>
__global__ __launch_bounds__(THREADS) void conv3x3s1_kernel(
    const float* __restrict__ X, const float* __restrict__ Wt, const float* __restrict__ bias,
    const float* __restrict__ addend, float* __restrict__ out, ConvShape g, int relu, float* __restrict__ stats)
{
    constexpr int APITCH = KContigPlanes<64, 16>::PITCH;     // 48 bytes: 16 bf16 + pad
    constexpr int APLANE = T3_AROWS * APITCH, AIMG = 3 * APLANE;
    typedef KContigPlanes<64, 16> BP3C;
    typedef KStridedPlanes<64, 16> BP3S;
    constexpr int BIMG = DGRAD ? BP3S::BYTES : BP3C::BYTES;
    constexpr int BPLANE = DGRAD ? BP3S::PLANE : BP3C::PLANE;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    unsigned char* A3 = reinterpret_cast<unsigned char*>(lds);       // [2][3 planes][66 rows][48]
    unsigned char* B3 = A3 + 2 * AIMG;                               // [2][3 planes]...
    unsigned char* dump = B3 + 2 * BIMG;                             // 3 x 512 bytes: where lanes without a second A row write

    const int W = g.Wi, H = g.Hi, Ca = g.Ci;                 // A-side image and channel count
    const int M = g.N * H * W, K = 9 * Ca;
    const int CC = Ca >> 4;                                  // 16-channel chunks
    const int tiles_n = (g.Co + 63) >> 6;
    const unsigned tile = xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (int)(tile / tiles_n) * 64, n0 = (int)(tile % tiles_n) * 64;
    const int u_begin = blockIdx.z * g.k_per_split, u_end = min(3 * CC, u_begin + g.k_per_split);      // units of this split
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;

    // ---- A staging: 66 rows x 4 chunks = 264 float4, thread tid takes chunk idx = tid and (tid < 8) idx = 256 + tid ----
    constexpr unsigned OOB = 0x80000000u;
    __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)X, 0, (int)min((long)M * Ca * 4, (long)0x7fffffff), 0x00020000);
    __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Wt, 0, (int)min((long)g.Co * K * 4, (long)0x7fffffff), 0x00020000);
    int a_off[2], a_ok[2], a_lds[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + 256 * i, row = idx >> 2, chunk = idx & 3;
        const bool rowok = idx < 4 * T3_AROWS;
        const int t = m0 - 1 + row;                          // aligned pixel of the row
        const bool tok = rowok && (unsigned)t < (unsigned)M;
        const int tt = tok ? t : 0;
        const int y = (tt / W) % H;
        a_ok[i] = (tok && y >= 1 ? 1 : 0) | (tok ? 2 : 0) | (tok && y + 1 < H ? 4 : 0);          // bit dyi: image row y + dyi - 1 exists
        a_off[i] = (t * Ca + chunk * 4) * 4;
        a_lds[i] = rowok ? row * APITCH + chunk * 8 : -1;
    }
    // ---- B staging (one float4 per thread and step), as in igemm_tile ----
    const int a_row = tid >> 2, a_chunk = tid & 3;           // forward: weight row n0 + a_row, k chunk a_chunk
    const int b_kk = tid >> 4, b_ch = tid & 15;              // dgrad: k row b_kk, columns n0 + 4 b_ch ..
    int b_off, b_lds;
    if (!DGRAD) {
        const int n = n0 + a_row;
        b_off = n < g.Co ? (n * K + a_chunk * 4) * 4 : (int)OOB;
        b_lds = a_row * BP3C::PITCH + a_chunk * 8;
    } else {
        const int n = n0 + b_ch * 4;
        b_off = n < g.Co ? (b_kk * 9 * g.Co + n) * 4 : (int)OOB;
        b_lds = b_kk * BP3S::PITCH + b_ch * 8;
    }
    // running unit decomposition of the LOADS (they run ahead of the multiplies): unit -> (dyi, cc)
    int la_dy = u_begin / CC, la_cc = u_begin - la_dy * CC, la_u = u_begin;           // next A block to load
    int lb_dy = la_dy, lb_cc = la_cc, lb_u = u_begin, lb_dx = 0;                    // next weight tile to load
    // (the 8 chunks past the first 256 belong to wave 0: the other waves skip them under a wave-uniform branch - done branch-free
    // with a dump slot, every thread paid a second split per unit and the kernel gained nothing over the generic one)
    const bool wave0 = __builtin_amdgcn_readfirstlane(wave) == 0;
    auto load_a = [&](f32x4 (&reg)[2]) {
        const bool uok = la_u < u_end;
        const int s_a = ((la_dy - 1) * W * Ca + la_cc * 16) * 4;
        {
            const bool ok = uok && ((a_ok[0] >> la_dy) & 1);
            reg[0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, ok ? a_off[0] + s_a : (int)OOB, 0, 0));
        }
        if (wave0) {
            const bool ok = uok && ((a_ok[1] >> la_dy) & 1);
            reg[1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, ok ? a_off[1] + s_a : (int)OOB, 0, 0));
        }
        ++la_u; ++la_cc;
        const int wrap = la_cc == CC;
        la_cc = wrap ? 0 : la_cc;
        la_dy += wrap;
    };
    auto load_b = [&](f32x4& reg) {
        const bool uok = lb_u < u_end;
        const int s_b = !DGRAD ? ((lb_dy * 3 + lb_dx) * Ca + lb_cc * 16) * 4
                               : ((lb_cc * 16 * 3 + (2 - lb_dy)) * 3 + (2 - lb_dx)) * g.Co * 4;
        reg = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, uok ? b_off + s_b : (int)OOB, 0, 0));
        ++lb_dx;
        const int w3 = lb_dx == 3;
        lb_dx = w3 ? 0 : lb_dx;
        lb_u += w3; lb_cc += w3;
        const int wrap = lb_cc == CC;
        lb_cc = wrap ? 0 : lb_cc;
        lb_dy += wrap;
    };
    auto store_a = [&](int aoff, const f32x4 (&reg)[2]) {
        store_split3<APLANE>(A3 + aoff, a_lds[0], reg[0]);
        if (wave0) {
            // second chunk: the 8 lanes that have one write it into the image, the others (an out-of-range load: zeros) into the dump
            unsigned h0, m0_, l0, h1, m1, l1;
            split3_pair(reg[1].x, reg[1].y, h0, m0_, l0);
            split3_pair(reg[1].z, reg[1].w, h1, m1, l1);
            const bool has = a_lds[1] >= 0;
            unsigned char* q = has ? A3 + aoff + a_lds[1] : dump + lane * 8;
            const int ps = has ? APLANE : 512;
            *reinterpret_cast<u32x2*>(q) = (u32x2){h0, h1};
            *reinterpret_cast<u32x2*>(q + ps) = (u32x2){m0_, m1};
            *reinterpret_cast<u32x2*>(q + 2 * ps) = (u32x2){l0, l1};
        }
    };
    auto store_b = [&](int boff, const f32x4& reg) { store_split3<BPLANE>(B3 + boff, b_lds, reg); };

    // accumulators start from bias (+ addend) when this launch is the final pass (igemm_tile)
    const bool final_pass = g.splits == 1;
    f32x16 acc[1][1];
    {
        const int n = n0 + wn + frag_col(lane);
        const bool nok = n < g.Co;
        const float bv = (final_pass && bias && nok) ? bias[n] : 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = m0 + wm + frag_row(lane, e);
            const bool ok = final_pass && addend && nok && m < M;
            acc[0][0][e] = bv + (ok ? addend[(size_t)(ok ? m : 0) * g.Co + (ok ? n : 0)] : 0.f);
        }
    }
    // per-lane border flags of this lane's A row (pixel m0 + wm + (lane & 31)): fixed over the K loop
    const int pr = m0 + wm + (lane & 31);
    const int px = (pr < M ? pr : 0) % W;
    const bool edge_l = px == 0, edge_r = px == W - 1;
    const bool any_l = __builtin_amdgcn_ballot_w64(edge_l) != 0, any_r = __builtin_amdgcn_ballot_w64(edge_r) != 0;

    if (u_begin < u_end) {
        f32x4 a_reg[2], b_set[3];
        load_a(a_reg);
#pragma unroll
        for (int d = 0; d < 3; ++d) load_b(b_set[d]);
        store_a(0, a_reg);
        load_a(a_reg);
        store_b(0, b_set[0]);
        load_b(b_set[0]);
        __syncthreads();
        int aoff = 0, boff = 0;                              // byte offsets of the A image / weight tile being multiplied
        const int r = lane & 31, hb = (lane >> 5) * 16;
        auto step = [&](auto DX) {
            constexpr int dxi = decltype(DX)::value;
            {
                Frag3 a[1], b[1];
                {
                    const unsigned char* p = A3 + aoff + (wm + r + dxi) * APITCH + hb;
                    a[0].hi = *reinterpret_cast<const bf16x8*>(p);
                    a[0].mid = *reinterpret_cast<const bf16x8*>(p + APLANE);
                    a[0].lo = *reinterpret_cast<const bf16x8*>(p + 2 * APLANE);
                }
                if (!DGRAD) read_kcontig3<1, BP3C::PITCH, BP3C::PLANE>(B3 + boff + wn * BP3C::PITCH, lane, 0, b);
                else read_kstrided3<1, BP3S::PITCH, BP3S::PLANE>(B3 + boff + wn * 2, lane, 0, b);
                if (dxi != 1 && (dxi == 0 ? any_l : any_r)) {  // the tap leaves the image row on this lane's pixel: a zero row
                    const bool z = dxi == 0 ? edge_l : edge_r;    // (wave-uniform skip: most waves of a wide image hold no border pixel)
                    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                    const u32x4 keep = z ? (u32x4){0u, 0u, 0u, 0u} : (u32x4){~0u, ~0u, ~0u, ~0u};
                    a[0].hi = __builtin_bit_cast(bf16x8, __builtin_bit_cast(u32x4, a[0].hi) & keep);
                    a[0].mid = __builtin_bit_cast(bf16x8, __builtin_bit_cast(u32x4, a[0].mid) & keep);
                    a[0].lo = __builtin_bit_cast(bf16x8, __builtin_bit_cast(u32x4, a[0].lo) & keep);
                }
                mma3_step<1, 1>(a, b, acc);
                // the next weight tile moves from its ring slot into the other LDS buffer; the slot takes the tile a unit ahead
                store_b(boff ^ BIMG, b_set[(dxi + 1) % 3]);
                load_b(b_set[(dxi + 1) % 3]);
                if (dxi == 2) {                               // ... and, on a unit's last step, the next A block
                    store_a(aoff ^ AIMG, a_reg);
                    load_a(a_reg);
                }
#pragma unroll
                for (int i = 0; i < 6; ++i) {                 // an MFMA, then a few of the split / address instructions, ...
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, dxi == 2 ? 14 : 8, 0);
                }
                __syncthreads();
                boff ^= BIMG;
            }
        };
        for (int u = u_begin; u < u_end; ++u) {
            step(std::integral_constant<int, 0>{});
            step(std::integral_constant<int, 1>{});
            step(std::integral_constant<int, 2>{});
            aoff ^= AIMG;
        }
    }

    // ---- per-channel statistics of the result for a following BatchNorm (igemm_tile) ----
    if (stats != nullptr && final_pass) {
        const int n = n0 + wn + frag_col(lane);
        float sm = 0.f, sq = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) { const float v = acc[0][0][e]; sm += v; sq += v * v; }
        sm += __shfl_xor(sm, 32, 64);
        sq += __shfl_xor(sq, 32, 64);
        if (lane < 32 && n < g.Co) {
            float* p = stats + (size_t)((m0 + wm) >> 5) * 2 * g.Co;
            p[n] = sm;
            p[g.Co + n] = sq;
        }
    }
    float* dst = out + (size_t)blockIdx.z * M * g.Co;
    const int n = n0 + wn + frag_col(lane);
    if (n < g.Co) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = m0 + wm + frag_row(lane, e);
            if (m < M) dst[(size_t)m * g.Co + n] = (final_pass && relu) ? fmaxf(acc[0][0][e], 0.f) : acc[0][0][e];
        }
    }
}

// out[i] = sum_z part[z][i] (+bias[i % ncols]) (relu)
// Every operand of an output element is fetched before the first add (the first eight partial sums branch-free - a
// split index past the end re-reads the last one - plus bias, addend and the old value): one memory latency per launch
// instead of one per split.  The additions keep their order (z ascending, then bias, addend, relu, old value).
// stats (optional; ncols a power of two <= 1024, no bias / relu): workgroup b also writes the per-column (sum, sum of squares)
// of its 1024 / ncols rows into stats[b][2 * ncols] - BatchNorm's statistics pass folded into the reduce.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                            const float* __restrict__ bias, const float* __restrict__ addend,
                                                            long total4, int ncols, int splits, int relu, int accumulate,
                                                            float* __restrict__ stats)
{
    __shared__ f32x4 red_s[2][256];
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (stats != nullptr) {                               // (every thread reaches the barrier below)
        const bool ok = i < total4;
        f32x4 s{0.f, 0.f, 0.f, 0.f};
        if (ok) {
            const f32x4* p = reinterpret_cast<const f32x4*>(part) + i;
            s = p[0];
            for (int z = 1; z < splits; ++z) s += p[(long)z * total4];
            reinterpret_cast<f32x4*>(out)[i] = s;
        }
        red_s[0][threadIdx.x] = s;
        red_s[1][threadIdx.x] = s * s;
        __syncthreads();
        const int c4 = ncols >> 2;                        // float4 columns; rows per workgroup = 256 / c4
        if ((int)threadIdx.x < c4) {
            f32x4 a = red_s[0][threadIdx.x], b = red_s[1][threadIdx.x];
            for (int r = c4; r < 256; r += c4) { a += red_s[0][r + threadIdx.x]; b += red_s[1][r + threadIdx.x]; }
            float* q = stats + (size_t)blockIdx.x * 2 * ncols + threadIdx.x * 4;
            *reinterpret_cast<f32x4*>(q) = a;
            *reinterpret_cast<f32x4*>(q + ncols) = b;
        }
        return;
    }
    if (i >= total4) return;
    const f32x4* p = reinterpret_cast<const f32x4*>(part) + i;
    const f32x4 zero{0.f, 0.f, 0.f, 0.f};
    f32x4 v[8];
#pragma unroll
    for (int z = 0; z < 8; ++z) v[z] = p[(long)min(z, splits - 1) * total4];
    const f32x4 bv = bias ? *reinterpret_cast<const f32x4*>(bias + (int)((i * 4) % ncols)) : zero;
    const f32x4 av = addend ? reinterpret_cast<const f32x4*>(addend)[i] : zero;
    const f32x4 ov = accumulate ? reinterpret_cast<const f32x4*>(out)[i] : zero;
    f32x4 s = v[0];
#pragma unroll
    for (int z = 1; z < 8; ++z)
        if (z < splits) s += v[z];
    for (int z = 8; z < splits; ++z) s += p[(long)z * total4];
    if (bias) s += bv;
    if (addend) s += av;
    if (relu) { s.x = fmaxf(s.x, 0.f); s.y = fmaxf(s.y, 0.f); s.z = fmaxf(s.z, 0.f); s.w = fmaxf(s.w, 0.f); }
    if (accumulate) s += ov;
    reinterpret_cast<f32x4*>(out)[i] = s;
}

// ---- stem helpers: NCHW (3 ch) -> NHWC padded to 4 channels; OHWI weight pad 3->4 and back -----------
__global__ void nchw3_to_nhwc4_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int HW)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)N * HW) return;
    const long n = i / HW, p = i - n * HW;
    const float* s = x + n * 3 * (long)HW + p;
    reinterpret_cast<f32x4*>(y)[i] = f32x4{s[0], s[HW], s[2 * (long)HW], 0.f};
}

__global__ void pad_channels_kernel(const float* __restrict__ src, float* __restrict__ dst, long rows, int cs, int cd)
{
    // dst[row][0..cd) = src[row][0..cs) zero-extended (cd > cs) or truncated (cd < cs)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cd) return;
    const long r = i / cd;
    const int c = (int)(i - r * cd);
    dst[i] = c < cs ? src[r * cs + c] : 0.f;
}

struct TileChoice { int bm, bn; };

// Modes 3 and 4 stage bf16 planes (three / one per operand).  The plan of mode 4 - tile, K-tile depth, ring depth - is mode 3's,
// decision for decision: at one clip these loops are bound by operand latency, which the arithmetic does not change.  The split count
// is not: plan_conv (profiles/README.md "bf16 inference" has what was measured).
inline bool staged(int mma) { return mma == 3 || mma == 4; }

TileChoice pick_tile(long M, long N)
{
    // Measured on MI355X (tests/tools/bench_conv.py): the problems of this path are small (a 5-frame clip), so what
    // matters is the number of co-resident workgroups per CU, not the tile's arithmetic intensity: 64x64 tiles with
    // the block count topped up to ~1250 by split-K beat the larger tiles on every trunk layer (72-80 us vs 85-130 us).
    const int mma = tuning().mma_mode;
    // (64x64 is the fastest tile of THIS kernel up to the 1200 rows of a batched clip; the Linear layers of that size whose launch
    // fits one round of tall tiles keep this plan's split count and leave for linrows.hip in pick_conv)
    if (staged(mma) && M <= 2048) return {64, 64};
    if (mma >= 1) {
        // split-bf16: the loop is bound by the operand split (VALU) and the LDS reads per MFMA, both of which shrink with
        // the wave tile - problems with enough tiles take the larger ones (bench_conv.py --mma --clips 8: 128x128 is
        // 15-20 % faster than 64x64 on the 8-clip trunk layers, and slower on every 1-clip layer)
        if (N >= 128 && ceil_div64(M, 128) * ceil_div64(N, 128) >= 300) return {128, 128};
        if (ceil_div64(M, 128) * ceil_div64(N, 64) >= 1250) return {128, 64};
    }
    return {64, 64};
}

struct ConvPlan { int bm, bn, splits; long tiles; };

// K-tile depth: 64 for the skinny (latency-bound) GEMMs of the lane head, 16 otherwise; split-bf16 on 64x64 tiles: 32
// (the MFMA work per barrier is 5x shorter there; measured 44-54 us vs 51-58 us on the trunk layers)
int k_tile_for(long M, int K, int ci, int bm, int bn)
{
    const int mma = tuning().mma_mode;
    // few-rows GEMMs (one frame of the lane head: 240 rows): deep K tiles.  With the frames of a clip batched (1200 rows) the
    // trunk plan wins in the staged-split arithmetic: 1024 -> 8192 174 vs 260 us, 4608 -> 1024 96 vs 146 us (bench_conv --only clipB)
    if (M <= (staged(mma) ? 256 : 2048) && K >= 64) return (staged(mma) && tuning().deep_kt3 == 32) ? 32 : 64;
    if (staged(mma)) return BK;                                          // 37 KB of LDS per 64x64 workgroup: four per CU
    if (mma >= 1 && bm == 64 && bn == 64 && ci % 32 == 0) return 32;
    return BK;
}

ConvPlan plan_conv(long M, int Co, int K, bool has_ws, size_t ws_bytes)
{
    const Tuning& tn = tuning();
    TileChoice t = pick_tile(M, Co);
    if (tn.force_bm) {
        t = {tn.force_bm, tn.force_bn};
        ConvPlan f{t.bm, t.bn, 1, ceil_div64(M, t.bm) * ceil_div64(Co, t.bn)};
        int splits = tn.force_splits > 0 ? tn.force_splits : 1;
        while (splits > 1 && (!has_ws || (size_t)splits * M * Co * sizeof(float) > ws_bytes)) --splits;
        f.splits = splits;
        return f;
    }
    ConvPlan p{t.bm, t.bn, 1, ceil_div64(M, t.bm) * ceil_div64(Co, t.bn)};
    // split K until ~1250 workgroups are in flight (about 5 per CU), keeping >= 256 of K per split
    // K-tile-64 plans (M <= 2048: the head GEMMs) hold 70 KB of LDS per workgroup = 2 workgroups per CU, so ~512 tiles already
    // fill the chip in one round and a split only adds the reduce pass (hyper-net 1024 -> 8192 at 240 rows: 54 vs 62 us)
    const bool deep = M <= (staged(tn.mma_mode) ? 256 : 2048) && K >= 64;
    // Mode 4 does not split K on its own.  The split count follows the tile count, i.e. the batch: a stream step (one frame) and a clip
    // (T frames) then sum an output's products in different groupings, the last bits differ, and the NEXT layer rounds them to bf16 -
    // a bf16 ulp (4e-3) apart where a value sits at a rounding boundary.  Unsplit, an output's accumulation chain (16-deep MFMA steps
    // in ascending K) is the same for every batch size, tile and K-tile depth: results are batch-invariant bit for bit.
    if (tn.mma_mode == 4 && !tn.bf16_splitk) return p;
    if (has_ws && p.tiles < (deep ? 400 : 900)) {
        int splits = (int)min((long)8, max((long)1, (1250 + p.tiles / 2) / p.tiles));
        while (splits > 1 && K / splits < 256) --splits;
        while (splits > 1 && (size_t)splits * M * Co * sizeof(float) > ws_bytes) --splits;
        p.splits = splits;
    }
    return p;
}

// extras: the launch has an addend or a statistics output (the host-only queries name the launch without them)
ConvPick pick_conv(const ConvShape& g, bool dgrad, bool has_ws, size_t ws_bytes, bool extras)
{
    const Tuning& tn = tuning();
    const long M = (long)g.N * g.Ho * g.Wo;
    const int K = g.R * g.S * g.Ci;
    const ConvPlan t = plan_conv(M, g.Co, K, has_ws, ws_bytes);
    ConvPick p{};
    p.dgrad = dgrad; p.bm = t.bm; p.bn = t.bn; p.splits = t.splits; p.tiles = t.tiles;
    // deep K tiles for skinny (latency-bound) problems: few row tiles and K long enough to fill them
    p.bkt = tn.force_kt ? tn.force_kt : k_tile_for(M, K, g.Ci, t.bm, t.bn);
    p.mma = tn.mma_mode;
    p.pf = staged(p.mma) ? ((tn.pf == 4 || tn.pf == 2) ? tn.pf : 1) : (p.mma == 0 && tn.pf == 4) ? 4 : 1;     // the instantiated ring depths
    // uniform-tap variant (the production tile only): the A-side channel count is a multiple of the K tile
    const bool uni = (g.Ci % p.bkt) == 0 && tn.uniform_tap;
    p.uni = uni && t.bm == 64 && t.bn == 64;
    p.buf = p.uni && g.in_dil == 1 && tn.buf_loads && staged(p.mma);
    // (the three-taps kernel exists in mode 3 only: mode 4 keeps these shapes on the generic kernel - or, one level up, on conv3p.hip)
    p.taps3 = tn.taps3 && p.mma == 3 && p.buf && g.R == 3 && g.S == 3 && g.stride == 1 && g.pad == 1 && g.Ho == g.Hi && g.Wo == g.Wi &&
              p.bkt == 16 && p.pf == 4 && g.Wi >= 2 && M * (long)g.Ci * 4 < 0x7fffffffL && (long)g.Co * K * 4 < 0x7fffffffL;
    // a Linear layer without epilogue extras: the tall-tile kernel where it applies to this plan's split count (linrows.hip)
    const bool linear = g.R == 1 && g.S == 1 && g.Hi == 1 && g.Wi == 1 && g.stride == 1 && g.pad == 0 && g.in_dil == 1;
    if (linear && !extras && (p.rows = linrows_wm(dgrad, M, K, g.Co, p.splits)) != 0) {
        p.bm = 160 * p.rows; p.bn = 128;
        p.tiles = ceil_div64(M, p.bm) * ceil_div64(g.Co, p.bn);
    }
    return p;
}

// the instantiation launch_conv's switch below launches for a pick, as rocprofv3 spells it
int conv_kernel_name(const ConvPick& p, char* name, int cap)
{
    static const char* const tf[2] = {"false", "true"};
    const int n = p.rows  ? (p.mma == 4 ? snprintf(name, (size_t)cap, LINROWS_BF16_NAME, p.rows)
                                        : snprintf(name, (size_t)cap, LINROWS_NAME, tf[p.dgrad], p.rows))
                : p.taps3 ? snprintf(name, (size_t)cap, "conv3x3s1_kernel<%s>", tf[p.dgrad])
                          : snprintf(name, (size_t)cap, "conv_igemm_kernel<%d, %d, %s, %d, %s, %d, %d, %s>", p.bm, p.bn, tf[p.dgrad], p.bkt,
                                     tf[p.uni], p.mma, p.pf, tf[p.buf]);
    return n < cap ? PHNET_OK : PHNET_ERR_ARG;
}

// The arithmetic rungs of the ladder in conv_igemm.h that this source builds: mode 3.  Only here is there a buffer-load
// instantiation to choose: pick_conv sets p.buf for mode 3 alone.
#define PHNET_LAUNCH_CONV___(DGRAD_, BM_, BN_, BKT_, UNI_, PF_)                                                         \
    do {                                                                                                                \
        if (p.buf) PHNET_LAUNCH_CONV____(DGRAD_, BM_, BN_, BKT_, UNI_, 3, PF_, UNI_);                                   \
        else PHNET_LAUNCH_CONV____(DGRAD_, BM_, BN_, BKT_, UNI_, 3, PF_, false);                                        \
    } while (0)
#define PHNET_LAUNCH_CONV_(DGRAD_, BM_, BN_, BKT_, UNI_)                                                                \
    do {                                                                                                                \
        if (p.pf == 4) PHNET_LAUNCH_CONV___(DGRAD_, BM_, BN_, BKT_, UNI_, 4);                                           \
        else if (p.pf == 2) PHNET_LAUNCH_CONV___(DGRAD_, BM_, BN_, BKT_, UNI_, 2);                                      \
        else PHNET_LAUNCH_CONV___(DGRAD_, BM_, BN_, BKT_, UNI_, 1);                                                     \
    } while (0)

// K range of one split of a pick: whole K tiles, the same number for every split (the last one takes what is left)
int k_per_split_of(const ConvPick& p, int K)
{
    const int ksteps = (K + p.bkt - 1) / p.bkt;
    return ((ksteps + p.splits - 1) / p.splits) * p.bkt;
}

template <bool DGRAD>
int launch_conv(const float* X, const float* W, const float* bias, const float* addend, float* out, float* workspace,
                size_t ws_bytes, ConvShape g, int relu, hipStream_t st, float* stats = nullptr)
{
    if (DGRAD && tuning().mma_mode == 4) return PHNET_ERR_ARG;      // the bf16 inference arithmetic is forward-only
    const ConvPick p = pick_conv(g, DGRAD, workspace != nullptr, ws_bytes, addend != nullptr || stats != nullptr);
    const long M = (long)g.N * g.Ho * g.Wo;
    const int K = g.R * g.S * g.Ci;
    const int splits = p.splits;
    g.splits = splits;
    float* dst = splits > 1 ? workspace : out;
    dim3 grid((unsigned)p.tiles, 1, (unsigned)splits);
    // ceil, so the last split can come out short or - with the 64-deep tile, where ksteps < splits * (splits - 1) happens (240 x
    // 1856 -> 2880: 29 steps, 7 splits of 5) - EMPTY: its workgroups skip the K loop and write zeros to their slice of the
    // partial sums (tests/gemm_cases.py "empty_split").  With 16-deep tiles plan_conv keeps >= 256 of K = 16 steps per split
    // and splits <= 8, so ksteps >= 16 * splits > splits * (splits - 1): no empty split there
    g.k_per_split = k_per_split_of(p, K);
    if (p.rows) {
        if (!linrows_launch(DGRAD, p.rows, X, W, bias, dst, M, K, g.Co, splits, g.k_per_split, relu, st)) return PHNET_ERR_LAUNCH;
    } else if (p.taps3) {
        const int units = 3 * (g.Ci / 16);
        // in units for this kernel.  The last split can be short (15 units over 2 splits), never empty: K / splits >= 256
        // (plan_conv) is units >= 5.34 * splits, and units < splits * (splits - 1) would then need splits > 6 - at 7 and 8
        // splits the only unit counts in range (39; 45, 48, 51, 54) leave the last split 3, 3, 6, 2 and 5 units
        g.k_per_split = (units + splits - 1) / splits;
        constexpr size_t lds_ = 2 * 3 * T3_AROWS * KContigPlanes<64, 16>::PITCH +
                                2 * (size_t)(DGRAD ? KStridedPlanes<64, 16>::BYTES : KContigPlanes<64, 16>::BYTES) + 3 * 512;
        hipLaunchKernelGGL((conv3x3s1_kernel<DGRAD>), grid, dim3(THREADS), lds_, st,
                           X, W, bias, addend, dst, g, relu, splits > 1 ? (float*)nullptr : stats);
    } else {
        const ConvLaunch a{X, W, bias, addend, dst, splits > 1 ? (float*)nullptr : stats, &g, relu, grid, st};
        if (p.mma == 4) launch_conv_bf16(p, a);
        else if (p.mma != 3) launch_conv_alt(p, a);
        else PHNET_LAUNCH_CONV_TILES(DGRAD);
    }
    if (splits > 1) {
        const long total4 = M * g.Co / 4;
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)ceil_div64(total4, 256)), dim3(256), 0, st,
                           workspace, out, bias, addend, total4, g.Co, splits, relu, 0, stats);
    }
    return phnet_launch_status();
}

}  // namespace

// Which tile / split-K factor / K tile phnet_conv2d_fwd runs a GEMM of M x Co x K with (a 1x1 convolution of K channels over M
// pixels; M < 2^31).  Answered by the pick_conv the launch itself calls.
PHNET_API int phnet_conv2d_plan(int64_t M, int32_t Co, int32_t K, uint64_t ws_bytes, int32_t* bm, int32_t* bn, int32_t* splits,
                                int32_t* k_tile)
{
    ConvShape g;
    if (M < 1 || M > 0x7fffffffL || Co < 1 || K < 1 || !bm || !bn || !splits || !k_tile) return PHNET_ERR_ARG;
    fwd_shape((int)M, 1, 1, K, Co, 1, 1, 1, 0, &g);
    const ConvPick p = pick_conv(g, false, ws_bytes > 0, (size_t)ws_bytes, false);
    *bm = p.bm; *bn = p.bn; *splits = p.splits; *k_tile = p.rows ? BK : p.bkt;
    return PHNET_OK;
}

// Host-only query: the kernel instantiation phnet_conv2d_fwd / _fwd_fused (dgrad = 0) or phnet_conv2d_dgrad (dgrad = 1) launches
// for the same shape arguments, as rocprofv3 spells it, and its split-K factor.
PHNET_API int phnet_conv2d_kernel(int32_t dgrad, int32_t N, int32_t Hi, int32_t Wi, int32_t Ci, int32_t Co, int32_t R, int32_t S,
                                  int32_t stride, int32_t pad, uint64_t ws_bytes, char* name, int32_t name_cap, int32_t* splits)
{
    ConvShape g;
    if (!conv_args_ok(N, Hi, Wi, Ci, Co, R, S, stride, pad) || N < 1 || !name || name_cap < 1 || !splits) return PHNET_ERR_ARG;
    if (dgrad && tuning().mma_mode == 4) return PHNET_ERR_ARG;      // forward-only arithmetic: there is no such launch
    if (dgrad ? (stride > 2 || !dgrad_shape(N, Hi, Wi, Ci, Co, R, S, stride, pad, &g)) : !fwd_shape(N, Hi, Wi, Ci, Co, R, S, stride, pad, &g))
        return PHNET_ERR_ARG;
    const ConvPick p = pick_conv(g, dgrad != 0, ws_bytes > 0, (size_t)ws_bytes, false);
    *splits = p.splits;
    return conv_kernel_name(p, name, name_cap);
}

// Forward convolution / linear.  x NHWC [N][Hi][Wi][Ci], w OHWI [Co][R][S][Ci], bias [Co] or NULL,
// y NHWC [N][Ho][Wo][Co].  Ci % 4 == 0, Co % 4 == 0.  workspace (optional, for split-K) is caller-allocated.
PHNET_API int phnet_conv2d_fwd(const float* x, const float* w, const float* bias, float* y,
                               int32_t N, int32_t Hi, int32_t Wi, int32_t Ci, int32_t Co, int32_t R, int32_t S,
                               int32_t stride, int32_t pad, int32_t relu,
                               void* workspace, uint64_t ws_bytes, void* stream)
{
    ConvShape g;
    if (!conv_args_ok(N, Hi, Wi, Ci, Co, R, S, stride, pad)) return PHNET_ERR_ARG;
    if (N == 0) return PHNET_OK;
    if (!x || !w || !y || !fwd_shape(N, Hi, Wi, Ci, Co, R, S, stride, pad, &g)) return PHNET_ERR_ARG;
    return launch_conv<false>(x, w, bias, nullptr, y, (float*)workspace, ws_bytes, g, relu, (hipStream_t)stream);
}

// Forward convolution with a fused epilogue: y = conv(x, w) + bias + addend, then ReLU (each part optional; addend shaped
// like y - the residual branch of a folded BatchNorm block in eval mode), and / or the per-channel batch statistics of y
// for a following BatchNorm: stats = phnet_conv2d_stats_blocks() rows of 2*Co floats (sum | sum of squares), the `partial`
// layout phnet_bn_finalize_partials reads.  stats needs bias == addend == NULL, relu == 0 and Co a power of two <= 1024.
static long conv_stats_blocks(long M, int Co, int K, bool has_ws, size_t ws_bytes)
{
    const ConvPlan t = plan_conv(M, Co, K, has_ws, ws_bytes);
    return t.splits > 1 ? ceil_div64(M * Co / 4, 256) : t.tiles / ceil_div64(Co, t.bn) * (t.bm / 32);
}

PHNET_API uint64_t phnet_conv2d_stats_blocks(int64_t M, int32_t Co, int32_t K, uint64_t ws_bytes)
{
    if (M < 1 || Co < 4 || K < 1) return 0;
    return (uint64_t)conv_stats_blocks((long)M, Co, K, ws_bytes > 0, (size_t)ws_bytes);
}

PHNET_API int phnet_conv2d_fwd_fused(const float* x, const float* w, const float* bias, const float* addend, float* y, float* stats,
                                     int32_t N, int32_t Hi, int32_t Wi, int32_t Ci, int32_t Co, int32_t R, int32_t S,
                                     int32_t stride, int32_t pad, int32_t relu,
                                     void* workspace, uint64_t ws_bytes, void* stream)
{
    ConvShape g;
    if (!conv_args_ok(N, Hi, Wi, Ci, Co, R, S, stride, pad)) return PHNET_ERR_ARG;
    if (stats && (bias || addend || relu || (Co & (Co - 1)) || Co > 1024)) return PHNET_ERR_ARG;
    if (N == 0) return PHNET_OK;
    if (!x || !w || !y || !fwd_shape(N, Hi, Wi, Ci, Co, R, S, stride, pad, &g)) return PHNET_ERR_ARG;
    return launch_conv<false>(x, w, bias, addend, y, (float*)workspace, ws_bytes, g, relu, (hipStream_t)stream, stats);
}

// Data gradient.  dy NHWC [N][Ho][Wo][Co], w OHWI [Co][R][S][Ci] (as used by the forward), dx NHWC [N][Hi][Wi][Ci].
// addend (optional, same shape as dx, may alias dx): dx = dgrad + addend  (residual-branch gradient).
PHNET_API int phnet_conv2d_dgrad(const float* dy, const float* w, const float* addend, float* dx,
                                 int32_t N, int32_t Hi, int32_t Wi, int32_t Ci, int32_t Co, int32_t R, int32_t S,
                                 int32_t stride, int32_t pad, void* workspace, uint64_t ws_bytes, void* stream)
{
    ConvShape g;
    if (!conv_args_ok(N, Hi, Wi, Ci, Co, R, S, stride, pad)) return PHNET_ERR_ARG;
    if (stride > 2) return PHNET_ERR_ARG;          // the data gradient supports strides 1 and 2 (all the model has)
    if (N == 0) return PHNET_OK;
    if (!dy || !w || !dx || !dgrad_shape(N, Hi, Wi, Ci, Co, R, S, stride, pad, &g)) return PHNET_ERR_ARG;
    return launch_conv<true>(dy, w, nullptr, addend, dx, (float*)workspace, ws_bytes, g, 0, (hipStream_t)stream);
}

// x NCHW [N][3][H][W] -> y NHWC [N][H][W][4] (4th channel zero): feeds the 7x7 stem.
PHNET_API int phnet_nchw3_to_nhwc4(const float* x, float* y, int32_t N, int32_t H, int32_t W, void* stream)
{
    if (N < 0 || H < 1 || W < 1) return PHNET_ERR_ARG;
    if (N == 0) return PHNET_OK;
    if (!x || !y) return PHNET_ERR_ARG;
    const long total = (long)N * H * W;
    hipLaunchKernelGGL(nchw3_to_nhwc4_kernel, dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       x, y, N, H * W);
    return phnet_launch_status();
}

// dst[rows][cd] <- src[rows][cs], zero-extending or truncating the innermost dimension.
PHNET_API int phnet_pad_channels(const float* src, float* dst, int64_t rows, int32_t cs, int32_t cd, void* stream)
{
    if (rows < 0 || cs < 1 || cd < 1) return PHNET_ERR_ARG;
    if (rows == 0) return PHNET_OK;
    if (!src || !dst) return PHNET_ERR_ARG;
    hipLaunchKernelGGL(pad_channels_kernel, dim3((unsigned)ceil_div64(rows * cd, 256)), dim3(256), 0, (hipStream_t)stream,
                       src, dst, (long)rows, cs, cd);
    return phnet_launch_status();
}
