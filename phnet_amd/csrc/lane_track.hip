// Lane identities on the device: the kept rows of phnet_lane_decode, frame after frame -> a stable id per lane, for B streams in
// one launch (DESIGN.md "Streaming path", lane identities).  Each stream keeps M track slots (id, missed, hits, extent, the xs of
// the last matched row) and the next id to hand out; the state lives in caller memory between launches.
//
// Rules, per stream and per frame, in this order (S offsets, L rows, M slots; a slot is LIVE when its id != 0):
//   1. extent of row r (the rule of lane_points.hip):  start = clamp(rint(double(r[2]) * (S-1)), 0, S-1),
//      end = min(start + rint(double(r[5])) - 1, S-1), in double.  Row d is TRACKABLE iff d < clamp(num, 0, L), r[2] and r[5]
//      are finite and end >= start.  Any other row gets track_id = -1, hits = 0 and never touches the state.
//   2. pair (trackable row d, live slot k):  lo = max(starts), hi = min(ends); skipped if hi < lo.  sum = f32 accumulation of
//      |row_x[i] - slot_x[i]|, i = lo..hi ascending, each term a < b ? b - a : a - b, no contraction (lanes_similar of
//      lane_nms.hip); cnt = hi - lo + 1.  CANDIDATE iff sum < thr * (float)cnt (one f32 multiply, strict); a NaN in the range
//      makes that false.
//   3. greedy, smallest mean first:  (sum_p, cnt_p) before (sum_q, cnt_q) iff double(sum_p) * cnt_q < double(sum_q) * cnt_p
//      (exact products, no division); ties: lower d, then lower k.  Pairs are taken in that order, skipping rows and slots
//      already taken.  A match copies the row's xs and extent into the slot, missed = 0, hits += 1; the row gets the slot's id
//      and hits.
//   4. every live slot not matched:  missed += 1; missed > max_age frees it (id = 0; nothing else of it changes).
//   5. every trackable unmatched row, ascending d:  takes the lowest free slot; if none, the slot with the largest missed among
//      those neither matched nor filled in this frame (ties: lowest slot; M >= L guarantees one).  id = next_id, next_id
//      advances and wraps from 2^31 - 1 to 1 (a stored next_id < 1 is read as 1); hits = 1, missed = 0, the row is copied in.
//
// One workgroup of ONE wavefront per stream; the wave walks the T frames of its stream in order.  Lane k owns slot k in
// registers for the whole launch, the slots' xs stay in LDS; both are loaded once and stored once, by that wave only, so no
// other workgroup ever sees a stream's state: no atomics, no cross-workgroup ordering, plain vector stores.  Per frame the rows
// are staged in LDS, lane p (striding by 64) evaluates pair p = d * M + k with its own ascending loop, and every greedy round is
// one wave argmin (DPP) under the ordering of rule 3 - p ascending IS (d, k) ascending, so the order is total and the minimum
// does not depend on the shape of the reduction.
#include "common.h"

namespace {

constexpr int kMaxTracks = 64;                // M: lane k owns slot k; L <= M
constexpr int kMaxOffsets = 256;              // S, as phnet_lane_points
constexpr int kMaxLdsWords = 15360;           // (L + M) * S + 2 * L * M dwords of dynamic LDS: 60 KiB

struct Cand { float sum; int cnt; int p; };   // cnt == 0: no candidate

// rule 3.  Sums of candidates are finite and >= 0, counts are in [1, 256]: both products are exact in double.
__device__ __forceinline__ bool before(const Cand& a, const Cand& b) {
    if (a.cnt == 0) return false;
    if (b.cnt == 0) return true;
    const double l = (double)a.sum * (double)b.cnt, r = (double)b.sum * (double)a.cnt;
    return l < r || (!(r < l) && a.p < b.p);
}

template <int CTRL>
__device__ __forceinline__ int dpp_move_i(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false); }

template <int CTRL>
__device__ __forceinline__ Cand first_step(const Cand& c) {
    const Cand o{dpp_move<CTRL>(c.sum), dpp_move_i<CTRL>(c.cnt), dpp_move_i<CTRL>(c.p)};
    return before(o, c) ? o : c;
}

// the first candidate of the wave under rule 3, in every lane (the sequence of wave_max; min is idempotent, so a lane
// whose DPP source is itself keeps its value).  All 64 lanes must be active.
__device__ __forceinline__ Cand wave_first(Cand c) {
    c = first_step<0xb1>(c);
    c = first_step<0x4e>(c);
    c = first_step<0x124>(c);
    c = first_step<0x128>(c);
    c = first_step<0x142>(c);
    c = first_step<0x143>(c);
    return Cand{__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c.sum), 63)),
                __builtin_amdgcn_readlane(c.cnt, 63), __builtin_amdgcn_readlane(c.p, 63)};
}

__device__ __forceinline__ int wave_max_i(int v) {
    v = max(v, dpp_move_i<0xb1>(v));
    v = max(v, dpp_move_i<0x4e>(v));
    v = max(v, dpp_move_i<0x124>(v));
    v = max(v, dpp_move_i<0x128>(v));
    v = max(v, dpp_move_i<0x142>(v));
    v = max(v, dpp_move_i<0x143>(v));
    return __builtin_amdgcn_readlane(v, 63);
}

// rule 2: the f32 sum of |a[i] - b[i]|, i = lo..hi ascending, in the arithmetic of lanes_similar (lane_nms.hip)
__device__ __forceinline__ float range_distance(const float* a, const float* b, int lo, int hi) {
#pragma clang fp contract(off)
    float dist = 0.0f;
    for (int i = lo; i <= hi; ++i) {
        const float x = a[i], y = b[i];
        dist += (x < y) ? (y - x) : (x - y);
    }
    return dist;
}

__device__ __forceinline__ bool is_candidate(float sum, float thr, int cnt) {
#pragma clang fp contract(off)
    return sum < thr * (float)cnt;
}

__global__ __launch_bounds__(64) void lane_track_kernel(const float* __restrict__ kept_rows, const int64_t* __restrict__ num,
                                                         int T, int L, int S, int M, float thr, int max_age,
                                                         int* __restrict__ trk_id, int* __restrict__ trk_missed,
                                                         int* __restrict__ trk_hits, int* __restrict__ trk_ext,
                                                         float* __restrict__ trk_x, int* __restrict__ next_id,
                                                         int* __restrict__ track_id, int* __restrict__ track_hits)
{
    extern __shared__ float lds[];
    float* s_trk = lds;                         // [M][S] the slots' xs: the state, for the whole launch
    float* s_row = s_trk + M * S;               // [L][S] this frame's rows
    float* s_sum = s_row + L * S;               // [L*M]  rule 2 of pair p = d * M + k
    int* s_cnt = reinterpret_cast<int*>(s_sum + L * M);      // [L*M]  0 = not a candidate
    __shared__ int s_id[kMaxTracks], s_start[kMaxTracks], s_end[kMaxTracks];      // what the pair lanes read of the slots
    __shared__ int d_start[kMaxTracks], d_end[kMaxTracks];                        // rule 1 per row; end < start = not trackable
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    const int W = 6 + S, pairs = L * M;

    // ---- the stream's state: lane k owns slot k ----
    int id = 0, missed = 0, hits = 0, tstart = 0, tend = -1;
    if (lane < M) {
        const size_t k = b * M + lane;
        id = trk_id[k]; missed = trk_missed[k]; hits = trk_hits[k];
        tstart = trk_ext[2 * k]; tend = trk_ext[2 * k + 1];
    }
#pragma unroll 1
    for (int i = lane; i < M * S; i += 64) s_trk[i] = trk_x[b * M * S + i];
    int nid = next_id[b];
    if (nid < 1) nid = 1;
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        const size_t f = b * T + t;
        const float* rows = kept_rows + f * L * W;
        const int64_t nf = num[f];
        const int kept = nf < 0 ? 0 : (nf > L ? L : (int)nf);

        // ---- rule 1, lane d; the slots as the pair lanes see them (a stored extent is never trusted as an LDS index) ----
        int ds = 0, de = -1;
        if (lane < kept) {
            const float r2 = rows[(size_t)lane * W + 2], r5 = rows[(size_t)lane * W + 5];
            if (fabsf(r2) <= 3.402823466e38f && fabsf(r5) <= 3.402823466e38f) {                        // false for NaN and +-inf
                const double sd = fmin(fmax(rint((double)r2 * (double)(S - 1)), 0.0), (double)(S - 1));
                const double ed = fmin(sd + rint((double)r5) - 1.0, (double)(S - 1));
                if (ed >= sd) { ds = (int)sd; de = (int)ed; }
            }
        }
        d_start[lane] = ds; d_end[lane] = de;
        if (lane < M) { s_id[lane] = id; s_start[lane] = max(tstart, 0); s_end[lane] = min(tend, S - 1); }
#pragma unroll 1
        for (int i = lane; i < L * S; i += 64) {
            const int d = i / S;
            s_row[i] = rows[(size_t)d * W + 6 + (i - d * S)];
        }
        __syncthreads();

        // ---- rule 2: one lane per pair ----
#pragma unroll 1
        for (int p = lane; p < pairs; p += 64) {
            const int d = p / M, k = p - d * M;
            const int a0 = d_start[d], a1 = d_end[d];
            float sum = 0.0f;
            int cnt = 0;
            if (a1 >= a0 && s_id[k] != 0) {
                const int lo = max(a0, s_start[k]), hi = min(a1, s_end[k]);
                if (hi >= lo) {
                    sum = range_distance(s_row + d * S, s_trk + k * S, lo, hi);
                    if (is_candidate(sum, thr, hi - lo + 1)) cnt = hi - lo + 1;
                }
            }
            s_sum[p] = sum; s_cnt[p] = cnt;
        }
        __syncthreads();

        // ---- rule 3: greedy rounds, wave-uniform ----
        unsigned long long row_taken = 0ull, slot_taken = 0ull;
        const unsigned long long trackable = __ballot(de >= ds);
        int my_id = -1, my_hits = 0;                                                                  // of row `lane`
        for (;;) {
            Cand c{0.0f, 0, 0x7fffffff};
#pragma unroll 1
            for (int p = lane; p < pairs; p += 64) {
                const int cnt = s_cnt[p];
                const int d = p / M, k = p - d * M;
                if (cnt == 0 || (((row_taken >> d) | (slot_taken >> k)) & 1ull)) continue;
                const Cand o{s_sum[p], cnt, p};
                if (before(o, c)) c = o;
            }
            c = wave_first(c);
            if (c.cnt == 0) break;
            const int d = c.p / M, k = c.p - d * M;
            row_taken |= 1ull << d; slot_taken |= 1ull << k;
#pragma unroll 1
            for (int i = lane; i < S; i += 64) s_trk[k * S + i] = s_row[d * S + i];
            if (lane == k) { tstart = d_start[d]; tend = d_end[d]; missed = 0; hits += 1; }
            const int kid = __shfl(id, k, 64), khits = __shfl(hits, k, 64);
            if (lane == d) { my_id = kid; my_hits = khits; }
        }

        // ---- rule 4 ----
        if (lane < M && id != 0 && !((slot_taken >> lane) & 1ull)) {
            missed += 1;
            if (missed > max_age) id = 0;
        }

        // ---- rule 5: births in ascending d ----
        unsigned long long born = trackable & ~row_taken, filled = 0ull;
#pragma unroll 1
        while (born) {
            const int d = __builtin_ctzll(born);
            born &= born - 1ull;
            const unsigned long long free_slots = __ballot(lane < M && id == 0);
            int k;
            if (free_slots) {
                k = __builtin_ctzll(free_slots);
            } else {
                const bool open = lane < M && !(((slot_taken | filled) >> lane) & 1ull);
                const int age = open ? max(missed, 0) : -1;
                const int oldest = wave_max_i(age);                                                   // >= 0: M >= L leaves a slot open
                k = __builtin_ctzll(__ballot(age == oldest));
            }
            filled |= 1ull << k;
#pragma unroll 1
            for (int i = lane; i < S; i += 64) s_trk[k * S + i] = s_row[d * S + i];
            if (lane == k) { id = nid; hits = 1; missed = 0; tstart = d_start[d]; tend = d_end[d]; }
            if (lane == d) { my_id = nid; my_hits = 1; }
            nid = nid == 0x7fffffff ? 1 : nid + 1;
        }
        if (lane < L) { track_id[f * L + lane] = my_id; track_hits[f * L + lane] = my_hits; }
        __syncthreads();                                                                              // the next frame restages the rows
    }

    if (lane < M) {
        const size_t k = b * M + lane;
        trk_id[k] = id; trk_missed[k] = missed; trk_hits[k] = hits;
        trk_ext[2 * k] = tstart; trk_ext[2 * k + 1] = tend;
    }
#pragma unroll 1
    for (int i = lane; i < M * S; i += 64) trk_x[b * M * S + i] = s_trk[i];
    if (lane == 0) next_id[b] = nid;
}

}  // namespace

// kept_rows [B][T][L][6+S], num i64 [B][T]; state trk_id / trk_missed / trk_hits i32 [B][M], trk_ext i32 [B][M][2], trk_x
// [B][M][S], next_id i32 [B]; out track_id / track_hits i32 [B][T][L].  1 <= L <= M <= 64, 2 <= S <= 256,
// (L + M) * S + 2 * L * M <= 15360, 1 <= T, 1 <= B < 2^31, max_age >= 0, thr finite and > 0.
PHNET_API int phnet_lane_track(const float* kept_rows, const int64_t* num, int64_t B, int32_t T, int32_t L, int32_t S, int32_t M,
                               float thr, int32_t max_age, int32_t* trk_id, int32_t* trk_missed, int32_t* trk_hits,
                               int32_t* trk_ext, float* trk_x, int32_t* next_id, int32_t* track_id, int32_t* track_hits, void* stream)
{
    if (!kept_rows || !num || !trk_id || !trk_missed || !trk_hits || !trk_ext || !trk_x || !next_id || !track_id || !track_hits)
        return PHNET_ERR_ARG;
    if (B < 1 || B > 0x7fffffffll || T < 1 || L < 1 || M < L || M > kMaxTracks || S < 2 || S > kMaxOffsets || max_age < 0)
        return PHNET_ERR_ARG;
    if (!(thr > 0.0f) || !(thr <= 3.402823466e38f)) return PHNET_ERR_ARG;                            // NaN, <= 0, +inf
    const int words = (L + M) * S + 2 * L * M;
    if (words > kMaxLdsWords) return PHNET_ERR_ARG;
    hipLaunchKernelGGL(lane_track_kernel, dim3((unsigned)B), dim3(64), (size_t)words * 4, (hipStream_t)stream, kept_rows, num,
                       (int)T, (int)L, (int)S, (int)M, thr, (int)max_age, trk_id, trk_missed, trk_hits, trk_ext, trk_x, next_id,
                       track_id, track_hits);
    return phnet_launch_status();
}
