// Guarded AdamW step over the flat arenas (include/phnet_hip.h, "guarded step", rules 1-8): a deterministic float64 sum of squares and
// a non-finite count of the gradient arena (phase A, HBM-bound: one read of the arena, 16-byte loads), one workgroup that turns them
// into norm / clip multiplier / skip decision and keeps the counters (phase B), and the AdamW launch that reads both from device
// memory.  No floating-point atomics, nothing to zero between steps, no host synchronisation: the three launches are capturable.
#include "common.h"
#include "adamw_update.h"
#include "../../include/phnet_hip.h"

namespace {
constexpr int NT = 256;
constexpr int WAVES = NT / 64;
constexpr int CHUNK = PHNET_GUARD_CHUNK;                 // elements per chunk = per workgroup of phase A
constexpr int CHUNK_VECS = CHUNK / 4;                    // 16-byte vectors per chunk
constexpr int IN_FLIGHT = 16;                            // vectors a lane loads before it consumes them
constexpr int ROUNDS = CHUNK_VECS / (NT * IN_FLIGHT);
constexpr int FIN_TILE = 4096;                           // chunk partials phase B stages in LDS at a time (32 KiB: 537 M elements a tile)
constexpr int FIN_BATCH = 32;                            // partials the adding lane reads from LDS ahead of its chain of additions
static_assert(CHUNK_VECS % (NT * IN_FLIGHT) == 0, "a chunk is a whole number of rounds");

__device__ __forceinline__ unsigned nonfinite_bits(float x) {       // exponent field all ones: an integer test no flag can fold away
    return (__builtin_bit_cast(unsigned, x) & 0x7f800000u) == 0x7f800000u;
}

// Rule 1, fixed by n and CHUNK alone.  Chunk c = elements [c CHUNK, min(n, (c+1) CHUNK)); vector q of it (q = 0 .. CHUNK/4-1) belongs
// to lane t = q % 256 of the workgroup; a lane keeps one float64 accumulator per vector component e and adds (double)g * (double)g of
// its vectors in ascending q (a float's square is exact in float64, so an fma and a multiply-add give the same bits; vectors past n add
// +0, which leaves the bits of a non-negative sum alone).  Lane: (a0 + a1) + (a2 + a3).  Wavefront: xor butterfly over lane distances
// 32, 16, 8, 4, 2, 1 (both partners compute x + y, so every lane ends with the same bits).  Chunk: ((w0 + w1) + w2) + w3.
template <bool FULL>
__device__ __forceinline__ void accumulate_chunk(const adamw_f32x4* __restrict__ gv, long nvec_left, int t, double (&acc)[4], unsigned& bad)
{
#pragma unroll 1
    for (int r = 0; r < ROUNDS; ++r) {
        adamw_f32x4 x[IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < IN_FLIGHT; ++u) {
            const int q = (r * IN_FLIGHT + u) * NT + t;
            x[u] = (FULL || q < nvec_left) ? gv[q] : adamw_f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < IN_FLIGHT; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)x[u][e];
                acc[e] += d * d;
                bad += nonfinite_bits(x[u][e]);
            }
    }
}

__global__ __launch_bounds__(NT) void guard_reduce_kernel(const float* __restrict__ g, long nvec, double* __restrict__ partial,
                                                          unsigned* __restrict__ count)
{
    __shared__ double wsum[WAVES];
    __shared__ unsigned wbad[WAVES];
    const int t = threadIdx.x;
    const long first = (long)blockIdx.x * CHUNK_VECS;
    const long left = nvec - first;                      // > 0: the grid is ceil(nvec / CHUNK_VECS)
    const adamw_f32x4* gv = reinterpret_cast<const adamw_f32x4*>(g) + first;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    unsigned bad = 0;
    if (left >= CHUNK_VECS) accumulate_chunk<true>(gv, left, t, acc, bad);      // uniform across the workgroup
    else accumulate_chunk<false>(gv, left, t, acc, bad);
    double s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s += __shfl_xor(s, d, 64);
        bad += __shfl_xor(bad, d, 64);
    }
    if ((t & 63) == 0) { wsum[t >> 6] = s; wbad[t >> 6] = bad; }
    __syncthreads();
    if (t == 0) {
        double cs = wsum[0];
        unsigned cb = wbad[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) { cs += wsum[w]; cb += wbad[w]; }
        partial[blockIdx.x] = cs;
        count[blockIdx.x] = cb;
    }
}

// Phase B, one workgroup: S = the chunk partials added in ascending chunk index by ONE lane (staged through LDS FIN_TILE at a time so
// that the loads are coalesced and the serial chain reads LDS), then rules 3-7.  stats: PHNET_GUARD_STATS_WORDS int64 words,
// word 0 = {f32 norm, f32 mult}, 1 = last step skipped, 2 = non-finite count, 3 = skipped steps in total (the only word read here).
__global__ __launch_bounds__(NT) void guard_finalize_kernel(const double* __restrict__ partial, const unsigned* __restrict__ count,
                                                            long nchunks, long long* __restrict__ stats, long long* __restrict__ step,
                                                            float max_norm, int flags, const float* __restrict__ grad_scale,
                                                            const float* __restrict__ found_inf)
{
    __shared__ double sp[FIN_TILE];
    __shared__ unsigned long long total_bad;
    const int t = threadIdx.x;
    double S = 0.0;
    unsigned long long mine = 0;
    if (t == 0) total_bad = 0;
    __syncthreads();
    for (long base = 0; base < nchunks; base += FIN_TILE) {
        const int m = (int)(nchunks - base < FIN_TILE ? nchunks - base : FIN_TILE);
#pragma unroll 4
        for (int k = t; k < m; k += NT) { sp[k] = partial[base + k]; mine += count[base + k]; }
        __syncthreads();
        if (t == 0) {                                    // the one serial chain of the step: LDS reads batched ahead of it
            int k = 0;
            for (; k + FIN_BATCH <= m; k += FIN_BATCH) {
                double x[FIN_BATCH];
#pragma unroll
                for (int u = 0; u < FIN_BATCH; ++u) x[u] = sp[k + u];
#pragma unroll
                for (int u = 0; u < FIN_BATCH; ++u) S += x[u];
            }
            for (; k < m; ++k) S += sp[k];
        }
        __syncthreads();
    }
    atomicAdd(&total_bad, mine);                         // an integer sum: any order gives the same count
    __syncthreads();
    if (t != 0) return;
    const unsigned long long nonfinite = total_bad;
    const float inv = grad_scale ? __fdiv_rn(1.0f, grad_scale[0]) : 1.0f;                  // rule 3
    const float norm = (float)(sqrt(S) * (double)inv);
    float coef = 1.0f;                                                                       // rule 4
    if (flags & PHNET_GUARD_CLIP) {
        const float c = __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f));
        coef = c > 1.0f ? 1.0f : c;                                                          // a NaN stays a NaN (torch.clamp(max=1))
    }
    const float mult = __fmul_rn(coef, inv);                                                 // rule 5
    const bool norm_bad = nonfinite_bits(norm);
    const bool inf_seen = found_inf && found_inf[0] != 0.0f;
    const bool skip = (flags & PHNET_GUARD_SKIP_NONFINITE) && (nonfinite > 0 || inf_seen || norm_bad);      // rule 6
    float* f = reinterpret_cast<float*>(stats);
    f[0] = norm;
    f[1] = mult;
    stats[1] = skip ? 1 : 0;
    stats[2] = (long long)nonfinite;
    stats[3] += skip ? 1 : 0;                                                                // rule 7
    if (!skip) step[0] += 1;                                                                 // rule 8
}

__global__ __launch_bounds__(NT) void adamw_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, long n4, long n_decay, const long long* __restrict__ step,
                                                           float lr, const float* __restrict__ lr_dev, float b1, float b2, float eps, float wd,
                                                           const float* __restrict__ mult, const long long* __restrict__ skip)
{
    if (skip[0] != 0) return;                            // uniform across the grid: a skipped step writes nothing
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= n4) return;
    adamw_update4<true>(p, g, m, v, i, n_decay, step, lr, lr_dev, b1, b2, eps, wd, mult[0]);
}
}  // namespace

PHNET_API int phnet_grad_guard(const float* g, int64_t n, void* workspace, uint64_t ws_bytes, int64_t* stats, int64_t* step,
                               float max_norm, int32_t flags, const float* grad_scale, const float* found_inf, void* stream)
{
    if (n < 0 || (n & 3) || (flags & ~(PHNET_GUARD_SKIP_NONFINITE | PHNET_GUARD_CLIP))) return PHNET_ERR_ARG;
    if (!(max_norm >= 0.0f)) return PHNET_ERR_ARG;                                          // negative or NaN
    if (!g || !workspace || !stats || !step) return PHNET_ERR_ARG;
    const int64_t nvec = n / 4, nchunks = ceil_div64(nvec, CHUNK_VECS);
    if (nchunks > 0x7fffffffLL) return PHNET_ERR_ARG;
    if (ws_bytes < (uint64_t)nchunks * PHNET_GUARD_WS_BYTES_PER_CHUNK) return PHNET_ERR_WORKSPACE;
    double* partial = (double*)workspace;                // nchunks float64 partials, then nchunks uint32 counts
    unsigned* count = (unsigned*)(partial + nchunks);
    if (nchunks)
        hipLaunchKernelGGL(guard_reduce_kernel, dim3((unsigned)nchunks), dim3(NT), 0, (hipStream_t)stream, g, (long)nvec, partial, count);
    hipLaunchKernelGGL(guard_finalize_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (const double*)partial, (const unsigned*)count,
                       (long)nchunks, (long long*)stats, (long long*)step, max_norm, (int)flags, grad_scale, found_inf);
    return phnet_launch_status();
}

PHNET_API int phnet_adamw_step_guarded(float* p, const float* g, float* m, float* v, int64_t n, int64_t n_decay, const int64_t* step,
                                       float lr, const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                                       const float* mult, const int64_t* skip, void* stream)
{
    if (n < 0 || (n & 3) || n_decay < 0 || n_decay > n) return PHNET_ERR_ARG;
    if (n == 0) return PHNET_OK;
    if (!p || !g || !m || !v || !step || !mult || !skip) return PHNET_ERR_ARG;
    hipLaunchKernelGGL(adamw_guarded_kernel, dim3((unsigned)ceil_div64(n / 4, NT)), dim3(NT), 0, (hipStream_t)stream, p, g, m, v,
                       (long)(n / 4), (long)n_decay, (const long long*)step, lr, lr_dev, beta1, beta2, eps, weight_decay, mult,
                       (const long long*)skip);
    return phnet_launch_status();
}
