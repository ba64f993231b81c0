// Forward and data gradient of a Linear layer over MANY rows with tall tiles and producer / consumer wavefronts (gfx950, bf16x3
// arithmetic):   y[m][n] = sum_k x[m][k] * w[n][k] (+ bias[n]) (ReLU)      and      dx[m][n] = sum_k dy[m][k] * w[k][n]
// (the hyper-network layers of the lane head, utils/dynamic_head.py:31-59, with the frames of a clip batched: 1200 rows x 1024 -> 8192
// and 1200 x 4608 -> 1024 forward, 1200 x 8192 -> 1024 backward, per stage).
//
// The generic kernel (conv_igemm_kernel, 64 x 64 tiles) re-reads 128 rows of K per 64 x 64 outputs and runs these layers at the L2
// rate that makes.  Here a workgroup owns 320 x 128 (unsplit) or 160 x 128 (split-K) outputs, chosen so that the
// launch is ONE round of 256 workgroups, one per CU: 4 or 8 consumer waves hold 5 x 1 accumulator fragments each (one B fragment serves
// five A fragments), only read fragments and multiply; 4 producer waves (one per SIMD) only load through a branch-free ring of four K
// steps of buffer loads, split into the three bf16 planes and fill the other LDS buffer one step ahead.  One barrier per step for all waves.
//
// The results are the generic kernel's bit for bit: an output element's bits depend only on its accumulation chain, and that is the
// chain of igemm_tile - v_mfma_f32_32x32x16_bf16 on 16-deep sub-steps in ascending K from the split's k_begin, lane (r, h) holding
// k = 8h .. 8h+7, the six terms in mma3_step's order, accumulators seeded with the bias (unsplit) or zeros (split), and the split
// of K and the reduce launch are conv.hip's own: pick_conv decides for this kernel, launch_conv launches it (linrows.h) and the
// generic entry points phnet_conv2d_fwd / _fwd_fused / _dgrad are the only way in.
#include <type_traits>
#include "conv_common.h"
#include "linrows.h"
#include "tuning.h"

using namespace igemm;

namespace {

constexpr int R_FM = 5;                                      // A fragments per consumer wave (160 rows)
constexpr int R_TN = 128;                                    // columns per workgroup: 4 consumer wave columns of one fragment each
constexpr int R_PRODUCERS = 4;                               // producer waves
constexpr int R_CUS = 256;                                   // a launch is planned as one round on the CUs of an MI355X

struct RowsShape {
    int M, K, N;                                             // rows, reduction depth, output columns
    int splits, k_per_split;                                 // k_per_split: multiple of BK
    int tiles_m;
};

// NP: bf16 planes per staged operand - 3: the exact split (mode 3), 1: the bf16 inference arithmetic (mode 4, forward only: one convert
// per element pair in the producers, one fragment read and one MFMA per product in the consumers; a third of the LDS)
template <bool DGRAD, int WM, int NP = 3> struct RowsCfg {
    static constexpr int TM = WM * R_FM * 32;                // 160 | 320 rows per workgroup
    static constexpr int CONSUMERS = 4 * WM;
    static constexpr int NT = (CONSUMERS + R_PRODUCERS) * 64;
    static constexpr int A_LOADS = (TM * 4 + R_PRODUCERS * 64 - 1) / (R_PRODUCERS * 64);     // float4 per producer thread and step: 3 | 5
    static constexpr int A_ROWS = A_LOADS * 64;              // rows of the staged A image (160 -> 192: the last 32 are staged as zeros, never read)
    static constexpr int B_LOADS = 2;                        // 128 x 16 floats
    static constexpr int PF = WM == 2 ? 3 : 4;               // producer register ring: K steps in flight per thread (7 | 5 float4 each)
    typedef KContigPlanes<A_ROWS, BK, NP> AP;
    typedef KContigPlanes<R_TN, BK, NP> BPC;
    typedef KStridedPlanes<R_TN, BK, NP> BPS;
    static constexpr int B_PITCH = DGRAD ? BPS::PITCH : BPC::PITCH;
    static constexpr int B_PLANE = DGRAD ? BPS::PLANE : BPC::PLANE;
    static constexpr int STAGE = AP::BYTES + NP * B_PLANE;   // A image | B image
    static constexpr int LDS = 2 * STAGE;                    // 92 KB | 129 KB (forward, three planes)
};

template <bool DGRAD, int WM, int NP>
__device__ __forceinline__ void linrows_tile(const float* __restrict__ A, const float* __restrict__ W, const float* __restrict__ bias,
                                             float* __restrict__ out, const RowsShape& g, int relu, unsigned char* lds_raw)
{
    typedef RowsCfg<DGRAD, WM, NP> C;
    typedef typename C::AP AP;
    static_assert(NP == 3 || (NP == 1 && !DGRAD), "three planes, or the forward-only one-plane arithmetic");
    const int M = g.M, K = g.K, N = g.N;
    const unsigned tile = xcd_remap(blockIdx.x, gridDim.x);
    // row tiles run fastest: the workgroups that share an L2 share weight columns and cover all rows
    const int m0 = (int)(tile % g.tiles_m) * C::TM, n0 = (int)(tile / g.tiles_m) * R_TN;
    const int k_begin = blockIdx.z * g.k_per_split, k_end = min(K, k_begin + g.k_per_split);
    const int nsteps = k_begin < k_end ? (k_end - k_begin) / BK : 0;                     // K and k_per_split are multiples of BK
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool final_pass = g.splits == 1;

    if (wave >= C::CONSUMERS) {
        // =============================== producers: global -> split -> LDS, one step ahead ===============================
        if (nsteps == 0) return;
        const int p = tid - C::CONSUMERS * 64;               // 0 .. 255
        const int a_row = p >> 2, a_chunk = p & 3;           // K-contiguous images: row a_row + 64 i, k chunk a_chunk
        constexpr unsigned OOB = 0x80000000u;                // past the end of both operands (< 2 GB each): the load returns zeros
        __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc((void*)A, 0, (int)min((long)M * K * 4, (long)0x7fffffff), 0x00020000);
        __amdgpu_buffer_rsrc_t rsrc_b = __builtin_amdgcn_make_buffer_rsrc((void*)W, 0, (int)min((long)N * K * 4, (long)0x7fffffff), 0x00020000);
        int a_off[C::A_LOADS], a_lds[C::A_LOADS], b_off[C::B_LOADS], b_lds[C::B_LOADS];
#pragma unroll
        for (int i = 0; i < C::A_LOADS; ++i) {
            const int row = a_row + 64 * i, m = m0 + row;
            a_off[i] = (row < C::TM && m < M) ? (m * K + a_chunk * 4) * 4 : (int)OOB;
            a_lds[i] = row * AP::PITCH + a_chunk * 8;
        }
#pragma unroll
        for (int i = 0; i < C::B_LOADS; ++i) {
            if (!DGRAD) {                                    // w[n][k]: rows = output columns, K contiguous
                const int n = n0 + a_row + 64 * i;
                b_off[i] = n < N ? (n * K + a_chunk * 4) * 4 : (int)OOB;
                b_lds[i] = (a_row + 64 * i) * C::B_PITCH + a_chunk * 8;
            } else {                                         // w[k][n]: 16 k rows x 32 float4 of columns
                const int idx = p + 256 * i, kk = idx >> 5, ch = idx & 31, n = n0 + ch * 4;
                b_off[i] = n < N ? (kk * N + n) * 4 : (int)OOB;
                b_lds[i] = kk * C::B_PITCH + ch * 8;
            }
        }
        constexpr int NL = C::A_LOADS + C::B_LOADS;
        f32x4 ring[C::PF][NL];
        int ld = 0;                                          // the next step to load (calls go through the steps in order)
        auto load_step = [&](f32x4 (&reg)[NL]) {
            const bool ok = ld < nsteps;                     // (uniform) past the end: zeros nobody multiplies
            const int s_a = (k_begin + BK * ld) * 4;
            const int s_b = DGRAD ? (k_begin + BK * ld) * N * 4 : s_a;
#pragma unroll
            for (int i = 0; i < C::A_LOADS; ++i)             // (an invalid row already sits at OOB; adding the small s_a keeps it there)
                reg[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, ok ? a_off[i] + s_a : (int)OOB, 0, 0));
#pragma unroll
            for (int i = 0; i < C::B_LOADS; ++i)
                reg[C::A_LOADS + i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_b, ok ? b_off[i] + s_b : (int)OOB, 0, 0));
            ++ld;
        };
        auto store_step = [&](int buf_off, const f32x4 (&reg)[NL]) {
#pragma unroll
            for (int i = 0; i < C::A_LOADS; ++i) {
                if constexpr (NP == 1) store_bf16(lds_raw + buf_off, a_lds[i], reg[i]);
                else store_split3<AP::PLANE>(lds_raw + buf_off, a_lds[i], reg[i]);
            }
#pragma unroll
            for (int i = 0; i < C::B_LOADS; ++i) {
                if constexpr (NP == 1) store_bf16(lds_raw + buf_off + AP::BYTES, b_lds[i], reg[C::A_LOADS + i]);
                else store_split3<C::B_PLANE>(lds_raw + buf_off + AP::BYTES, b_lds[i], reg[C::A_LOADS + i]);
            }
        };
#pragma unroll
        for (int d = 0; d < C::PF; ++d) load_step(ring[d]);
        store_step(0, ring[0]);
        load_step(ring[0]);
        __syncthreads();                                     // step 0 is staged
        int o_st = C::STAGE;
        // iteration t (the consumers multiply step t) stages step t + 1 out of ring[(t + 1) % PF] into the other buffer and reloads that
        // entry with step t + 1 + PF; the main loop is free of conditions (a branch around a load makes hipcc drain the ring, wgrad3s.hip)
        bool reload = true;
        auto body = [&](auto U, int) {
            constexpr int slot = (decltype(U)::value + 1) % C::PF;
            store_step(o_st, ring[slot]);                    // (on the last step: a block nobody reads)
            if (reload) load_step(ring[slot]);
            __syncthreads();
            o_st = C::STAGE - o_st;
        };
        int t = 0;
        for (; t + C::PF <= nsteps; t += C::PF) unroll_iterations<C::PF>(body, t);
        reload = false;
        tail_iterations<C::PF - 1>(body, t, nsteps);
        return;
    }

    // ======================================= consumers: fragments -> MFMAs =======================================
    const int wm = (wave >> 2) * (R_FM * 32), wn = (wave & 3) * 32;
    const int n = n0 + wn + frag_col(lane);
    const bool nok = n < N;
    f32x16 acc[R_FM][1];
    {
        const float bv = (final_pass && bias && nok) ? bias[n] : 0.f;
#pragma unroll
        for (int f = 0; f < R_FM; ++f)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[f][0][e] = bv + 0.f;          // as igemm_tile seeds them (bias + no addend)
    }
    if (nsteps > 0) {
        const unsigned char* a_src = lds_raw + wm * AP::PITCH;
        const unsigned char* b_src = lds_raw + AP::BYTES + (DGRAD ? wn * 2 : wn * C::B_PITCH);
        int o = 0;
        __syncthreads();                                     // step 0 is staged
        for (int t = 0; t < nsteps; ++t) {
            if constexpr (NP == 1) {
                bf16x8 fa[R_FM], fb[1];
                read_kcontig1<1, C::B_PITCH>(b_src + o, lane, 0, fb);
                read_kcontig1<R_FM, AP::PITCH>(a_src + o, lane, 0, fa);
                mma1_step<R_FM, 1>(fa, fb, acc);
            } else {
                Frag3 fa[R_FM], fb[1];
                if (!DGRAD) read_kcontig3<1, C::B_PITCH, C::B_PLANE>(b_src + o, lane, 0, fb);
                else read_kstrided3<1, C::B_PITCH, C::B_PLANE>(b_src + o, lane, 0, fb);
                read_kcontig3<R_FM, AP::PITCH, AP::PLANE>(a_src + o, lane, 0, fa);
                mma3_step<R_FM, 1>(fa, fb, acc);
            }
            __syncthreads();
            o = C::STAGE - o;
        }
    }
    // ---- epilogue: bias (seeded) / ReLU, or raw partial sums into slab blockIdx.z; rows >= M and columns >= N are never stored ----
    float* dst = out + (size_t)blockIdx.z * M * N;
    if (nok) {
#pragma unroll
        for (int f = 0; f < R_FM; ++f)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wm + 32 * f + frag_row(lane, e);
                if (m < M) dst[(size_t)m * N + n] = (final_pass && relu) ? fmaxf(acc[f][0][e], 0.f) : acc[f][0][e];
            }
    }
}

template <bool DGRAD, int WM>
__global__ __launch_bounds__((RowsCfg<DGRAD, WM>::NT)) void linrows_kernel(const float* __restrict__ A, const float* __restrict__ W,
                                                                         const float* __restrict__ bias, float* __restrict__ out,
                                                                         RowsShape g, int relu)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];               // [buffer 0..1][A planes | B planes]
    linrows_tile<DGRAD, WM, 3>(A, W, bias, out, g, relu, lds_raw);
}

// the forward in the bf16 inference arithmetic (mode 4): same tiles, same schedule, one plane
template <int WM>
__global__ __launch_bounds__((RowsCfg<false, WM>::NT)) void linrows_bf16_kernel(const float* __restrict__ A, const float* __restrict__ W,
                                                                              const float* __restrict__ bias, float* __restrict__ out,
                                                                              RowsShape g, int relu)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    linrows_tile<false, WM, 1>(A, W, bias, out, g, relu, lds_raw);
}

inline long cdiv(long a, long b) { return (a + b - 1) / b; }

// what the kernel itself needs: a staged arithmetic (mode 3, or mode 4 for the forward), whole 16-deep steps, float4 columns, 32-bit byte offsets with room for
// the rows of a ragged last tile
bool rows_ok(bool dgrad, long M, int K, int N)
{
    const int mma = tuning().mma_mode;
    return (mma == 3 || (mma == 4 && !dgrad)) && M >= 1 && K >= BK && (K % BK) == 0 && N >= 4 && (N & 3) == 0 &&
           (M + 320) * K * 4 < 0x7fffffffL && (long)N * K * 4 < 0x7fffffffL && (M + 320) * N * 4 < 0x7fffffffL;
}

template <bool DGRAD, int WM>
bool launch_rows_as(const float* a, const float* w, const float* bias, float* dst, const RowsShape& g, int relu, dim3 grid, hipStream_t st)
{
    typedef RowsCfg<DGRAD, WM> C;
    static bool attr = false;
    if (!attr && !(attr = phnet_allow_dynamic_lds({(const void*)linrows_kernel<DGRAD, WM>}, C::LDS))) return false;
    hipLaunchKernelGGL((linrows_kernel<DGRAD, WM>), grid, dim3(C::NT), C::LDS, st, a, w, bias, dst, g, relu);
    return true;
}

template <int WM>
bool launch_rows_bf16(const float* a, const float* w, const float* bias, float* dst, const RowsShape& g, int relu, dim3 grid, hipStream_t st)
{
    typedef RowsCfg<false, WM, 1> C;                         // 31 KB | 43 KB: no opt-in needed
    static_assert(C::LDS <= 64 * 1024, "fits the default dynamic LDS limit");
    hipLaunchKernelGGL((linrows_bf16_kernel<WM>), grid, dim3(C::NT), C::LDS, st, a, w, bias, dst, g, relu);
    return true;
}

}  // namespace

// ---- what csrc/conv.hip takes from here (linrows.h) --------------------------------------------------------------------------------
// Mode 1, the shapes this kernel was measured faster at than the generic one: many-row layers - never the
// few-rows ones, which have kernels of their own - with whole column tiles, a deep reduction, a plan nobody forced, and a launch that
// is one (nearly) full round of the CUs.
int linrows_wm(bool dgrad, long M, int K, int N, int splits)
{
    const Tuning& tn = tuning();
    if (!tn.linrows || !rows_ok(dgrad, M, K, N)) return 0;
    const int wm = splits == 1 ? 2 : 1;                     // 320 rows unsplit, 160 where split-K multiplies the workgroups
    if (tn.linrows == 2) return wm;
    if (tn.force_bm || tn.force_kt || M <= 256 || M > 2048 || (N % R_TN) != 0 || K < 1024) return 0;
    const long wgs = cdiv(M, wm * R_FM * 32) * cdiv(N, R_TN) * splits;
    return wgs > R_CUS * 3 / 4 && wgs <= R_CUS ? wm : 0;
}

bool linrows_launch(bool dgrad, int wm, const float* a, const float* w, const float* bias, float* dst, long M, int K, int N, int splits,
                    int k_per_split, int relu, hipStream_t st)
{
    const long tiles_m = cdiv(M, wm * R_FM * 32);
    const RowsShape g{(int)M, K, N, splits, k_per_split, (int)tiles_m};
    const dim3 grid((unsigned)(tiles_m * cdiv(N, R_TN)), 1, (unsigned)splits);
    if (tuning().mma_mode == 4) {
        if (dgrad) return false;                             // (never picked: linrows_wm)
        return wm == 2 ? launch_rows_bf16<2>(a, w, bias, dst, g, relu, grid, st) : launch_rows_bf16<1>(a, w, bias, dst, g, relu, grid, st);
    }
    if (dgrad) return wm == 2 ? launch_rows_as<true, 2>(a, w, bias, dst, g, relu, grid, st) : launch_rows_as<true, 1>(a, w, bias, dst, g, relu, grid, st);
    return wm == 2 ? launch_rows_as<false, 2>(a, w, bias, dst, g, relu, grid, st) : launch_rows_as<false, 1>(a, w, bias, dst, g, relu, grid, st);
}
