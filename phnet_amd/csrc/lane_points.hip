// Lane polylines on the device: the kept rows of phnet_lane_decode -> the (x, y) points of every lane, packed per frame, in one
// launch for all frames (DESIGN.md "Streaming path", polylines).  Replaces the host loop DetNetV2.predictions_to_pred
// (libs/models/Router4OL.py:394-435: .item() calls, a numpy reverse-cumprod, boolean indexing, one scipy spline per lane) for
// callers that want points, and leaves them where a device-side consumer can read them.
//
// Rules, for a row r of S offsets (n_strips = S - 1), exactly the host's:
//   start = clamp(rint(double(r[2]) * n_strips), 0, n_strips)       product in double, half to even (Python round on a float)
//   end   = min(start + rint(double(r[5])) - 1, S - 1)              in double: no 32-bit overflow
//   e     = end + 1;  e < 0 -> max(S + e, 0)                        the Python slice xs[end + 1:] with a negative bound
//   lo    = 1 + the highest i < start whose x is not in [0, 1]      (0 when there is none): the contiguous extension below start
//   entry i survives iff lo <= i < e and x[i] >= 0                  NaN never survives; x > 1 inside [start, end] does
//   survivors are emitted in DESCENDING i as (x[i], prior_ys[i]); a row with <= 1 survivor is not a lane.
// A row whose r[2] or r[5] is NaN / +-inf is not a lane (the host code raises on it).
// Values are copied, never computed: the output is the host's float64 result bit for bit after widening.
//
// One workgroup per frame, one wavefront per kept slot (min(L, 16) waves, each takes slots w, w + 16, ...).  Phase 1: a wave
// loads its row, 64 offsets per round, and reduces the tests to ballots: the survivor mask of each round and its popcount go to
// LDS.  Phase 2 (after one barrier): the packed position of a slot is the number of lanes among the slots before it - one ballot
// over the L counts - and the position of a survivor is the number of survivors above it (mbcnt on its round's mask + the
// popcounts of the later rounds).  Every element of every output is written exactly once by plain vector stores: no atomics, and
// a replayed graph never shows a stale lane.
#include "common.h"

namespace {

constexpr int kMaxLanes = 64;                 // L: one ballot packs a frame (phnet_lane_decode: top_k <= 64)
constexpr int kRounds = 4;                    // 64 offsets per round
constexpr int kMaxOffsets = 64 * kRounds;     // S <= 256 (phnet_lane_decode: n_offsets <= 250)
constexpr int kMaxWaves = 16;

__device__ __forceinline__ int bits_below_lane(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__global__ __launch_bounds__(64 * kMaxWaves) void lane_points_kernel(const float* __restrict__ kept_rows,
                                                                      const int64_t* __restrict__ num,
                                                                      const float* __restrict__ prior_ys, int L, int S,
                                                                      float2* __restrict__ points, int* __restrict__ count,
                                                                      int* __restrict__ lanes_num, int* __restrict__ slot)
{
    __shared__ unsigned long long s_mask[kMaxLanes][kRounds];
    __shared__ int s_cnt[kMaxLanes];
    const size_t f = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int W = 6 + S, n_strips = S - 1;
    const int64_t nf = num[f];
    const int kept = nf < 0 ? 0 : (nf > L ? L : (int)nf);
    const float* rows = kept_rows + f * (size_t)L * W;

    // ---- phase 1: survivor masks and counts of every slot ----
    for (int k = wave; k < L; k += waves) {
        const float* r = rows + (size_t)k * W;
        unsigned long long m[kRounds] = {0ull, 0ull, 0ull, 0ull};
        int total = 0;
        if (k < kept) {
            const float r2 = r[2], r5 = r[5];
            const bool finite = fabsf(r2) <= 3.402823466e38f && fabsf(r5) <= 3.402823466e38f;      // false for NaN and +-inf
            if (finite) {
                double sd = rint((double)r2 * (double)n_strips);
                sd = fmin(fmax(sd, 0.0), (double)n_strips);
                const int start = (int)sd;
                double ed = fmin(sd + rint((double)r5) - 1.0, (double)(S - 1)) + 1.0;
                if (ed < 0.0) ed = fmax((double)S + ed, 0.0);
                const int e = (int)ed;                                                                // 0 <= e <= S
                float x[kRounds];
                int hb = -1;                                                                          // highest out-of-image i < start
#pragma unroll
                for (int c = 0; c < kRounds; ++c) {
                    const int i = c * 64 + lane;
                    x[c] = (c * 64 < S && i < S) ? r[6 + i] : -2.0f;
                    const unsigned long long bad = __ballot(i < start && !(x[c] >= 0.0f && x[c] <= 1.0f));
                    if (bad) hb = c * 64 + 63 - __builtin_clzll(bad);
                }
#pragma unroll
                for (int c = 0; c < kRounds; ++c) {
                    const int i = c * 64 + lane;
                    m[c] = __ballot(i > hb && i < e && x[c] >= 0.0f);
                    total += __popcll(m[c]);
                }
            }
        }
        if (lane < kRounds) s_mask[k][lane] = lane == 0 ? m[0] : lane == 1 ? m[1] : lane == 2 ? m[2] : m[3];
        if (lane == 0) s_cnt[k] = total;
    }
    __syncthreads();

    // ---- phase 2: pack the lanes of the frame, emit the points ----
    const unsigned long long is_lane = __ballot(lane < L && s_cnt[lane < L ? lane : 0] > 1);
    const int n_lanes = __popcll(is_lane);
    if (threadIdx.x == 0) lanes_num[f] = n_lanes;
    float2* pts = points + f * (size_t)L * S;
    const float2 zero = make_float2(0.f, 0.f);
    for (int k = wave; k < L; k += waves) {
        if (!((is_lane >> k) & 1ull)) continue;                                                      // wave-uniform
        const int p = __popcll(is_lane & ((1ull << k) - 1ull));
        const float* r = rows + (size_t)k * W;
        float2* dst = pts + (size_t)p * S;
        const int total = s_cnt[k];
        int above = total;                                                                            // survivors in this and later rounds
#pragma unroll
        for (int c = 0; c < kRounds; ++c) {
            const unsigned long long mc = s_mask[k][c];
            const int i = c * 64 + lane;
            above -= __popcll(mc);                                                                    // survivors in later rounds only
            if ((mc >> lane) & 1ull)
                dst[above + __popcll(mc) - bits_below_lane(mc) - 1] = make_float2(r[6 + i], prior_ys[i]);
        }
        for (int j = total + lane; j < S; j += 64) dst[j] = zero;
        if (lane == 0) { count[f * L + p] = total; slot[f * L + p] = k; }
    }
    for (int p = n_lanes + wave; p < L; p += waves) {                                                 // unused packed slots
        float2* dst = pts + (size_t)p * S;
        for (int j = lane; j < S; j += 64) dst[j] = zero;
        if (lane == 0) { count[f * L + p] = 0; slot[f * L + p] = -1; }
    }
}

}  // namespace

// kept_rows [F][L][6+S] as phnet_lane_decode writes them, num i64 [F], prior_ys [S] -> points [F][L][S][2], count i32 [F][L],
// lanes_num i32 [F], slot i32 [F][L].  1 <= L <= 64, 2 <= S <= 256, 1 <= F < 2^31.
PHNET_API int phnet_lane_points(const float* kept_rows, const int64_t* num, const float* prior_ys, int64_t F, int32_t L, int32_t S,
                                float* points, int32_t* count, int32_t* lanes_num, int32_t* slot, void* stream)
{
    if (!kept_rows || !num || !prior_ys || !points || !count || !lanes_num || !slot) return PHNET_ERR_ARG;
    if (F < 1 || F > 0x7fffffffll || L < 1 || L > kMaxLanes || S < 2 || S > kMaxOffsets) return PHNET_ERR_ARG;
    const int waves = L < kMaxWaves ? L : kMaxWaves;
    hipLaunchKernelGGL(lane_points_kernel, dim3((unsigned)F), dim3(64 * waves), 0, (hipStream_t)stream, kept_rows, num, prior_ys,
                       (int)L, (int)S, reinterpret_cast<float2*>(points), count, lanes_num, slot);
    return phnet_launch_status();
}
