// Device-side body of the label assignment (see assign.hip): one workgroup of 256 (QUAD = 1) or 1024 (QUAD = 4) threads, callable
// from other kernels.
#pragma once
#include "common.h"

namespace phassign {

constexpr int NT = 256;
constexpr int MAXL = 4;
constexpr int CAND = NT / 64;                        // rows of one column that a lane of the column's wave looks at (N <= NT)

template <int V> struct PfTag { static constexpr int value = V; };

// The maxima of three values over the workgroup in one exchange: a wave reduction each, one LDS write per wave, one barrier.
// fmaxf over a set does not depend on the order.  `red` is written nowhere else, and every later use of this function lies
// several barriers behind the reads below.
template <int WAVES>
__device__ __forceinline__ void block_max3(float& a, float& b, float& c, float (*red)[3]) {
    a = wave_max(a); b = wave_max(b); c = wave_max(c);
    if ((threadIdx.x & 63) == 0) {
        float* r = red[threadIdx.x >> 6];
        r[0] = a; r[1] = b; r[2] = c;
    }
    __syncthreads();
    a = red[0][0]; b = red[0][1]; c = red[0][2];
#pragma unroll
    for (int i = 1; i < WAVES; ++i) { a = fmaxf(a, red[i][0]); b = fmaxf(b, red[i][1]); c = fmaxf(c, red[i][2]); }
}

// Number of the S label columns inside [0, img_w), counted by the calling wave (all 64 lanes active) and returned to each of its
// lanes: 64 columns per ballot.  An integer count, exact in any order.  tx: one row of t_x (256 entries, S <= 250).
__device__ __forceinline__ float wave_len(const float* tx, int S, float img_w) {
    const int lane = threadIdx.x & 63;
    int n = 0;
    for (int k0 = 0; k0 < S; k0 += 64) {
        const int k = k0 + lane;                     // k0 <= 192: k < 256
        const float t = tx[k];
        n += __popcll(__ballot(k < S && !((t < 0.f) || (t >= img_w))));
    }
    return (float)n;
}

// The best (value, index) pair of the wave on the DPP data path (the sequence of wave_max; all 64 lanes active), returned to every
// lane.  LESS: the lowest value, else the highest; equal values go to the lower index.  The order is total on the pairs that
// get here (no NaN: a lane never picks one up), so the result does not depend on the pairing of the lanes.
template <int CTRL, bool LESS>
__device__ __forceinline__ void arg_best_step(float& bv, int& bi) {
    const float ov = dpp_move<CTRL>(bv);
    const int oi = __builtin_amdgcn_update_dpp(bi, bi, CTRL, 0xf, 0xf, false);
    const bool take = LESS ? (ov < bv || (ov == bv && oi < bi)) : (ov > bv || (ov == bv && oi < bi));
    bv = take ? ov : bv;
    bi = take ? oi : bi;
}
template <bool LESS>
__device__ __forceinline__ void wave_arg_best(float& bv, int& bi) {
    arg_best_step<0xb1, LESS>(bv, bi);       // quad_perm [1,0,3,2]
    arg_best_step<0x4e, LESS>(bv, bi);       // quad_perm [2,3,0,1]
    arg_best_step<0x124, LESS>(bv, bi);      // row_ror 4
    arg_best_step<0x128, LESS>(bv, bi);      // row_ror 8
    arg_best_step<0x142, LESS>(bv, bi);      // row_bcast 15
    arg_best_step<0x143, LESS>(bv, bi);      // row_bcast 31: lane 63 holds the best of all 64 lanes
    bv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bv), 63));
    bi = __builtin_amdgcn_readlane(bi, 63);
}

// QUAD = 4: the workgroup has 4 x NT threads and the cost phase gives every (anchor, label) pair its own thread (with one thread
// per anchor the 4 waves of the single workgroup sit alone on their SIMDs and the 4 S-long accumulation chains of a thread run at
// the latency of dependent VALU issue: 14 of the kernel's 23 us); the matching phases use the first NT threads as before.
// MANY = false: the one-to-one assignment of `assign` (dynamic_assign.py:128-190; focal_alpha 0.25).
// MANY = true: `assignOne2Many` (dynamic_assign.py:292-357; focal_alpha 0.5): label j wants k_j = max(1, int(sum of its 4 largest
// line IoUs)) anchors; rounds of the exact matching over ALL valid labels, each round keeps the pairs whose POSITION p in the
// row-sorted pair list has k_p > 0 (as shipped: the per-label mask indexes the pair list, :351), retires their rows, decrements
// the positive k's.  many_rows / many_cols [MAXL*MAXL] (-1 padded; cols = original label rows), many_n = number of pairs.
// sorted_lds (optional, MANY = false): LDS [MAXL], receives what rows_sorted receives (-1 padded to MAXL) for the caller to read after
// the barrier that ends this function.
//
// One workgroup pays every dependent trip to global memory in full, so the function makes ONE: the anchor's class logit, start and
// angle and - where the row fits in registers (6 + S even, S <= 72) - all its x columns are requested before the label rows are
// staged into LDS, and nothing else is read from global memory afterwards.  MAXPF = 18 caps the register-held row at 36 columns for
// a caller that keeps registers of its own across the call.
template <bool MANY = false, int QUAD = 1, int MAXPF = 36>
__device__ __forceinline__ void lane_assign_block(
    const float* __restrict__ pred, const float* __restrict__ tgt, int N, int L, int S, float img_w, float img_h,
    int64_t* __restrict__ rows_by_col, int64_t* __restrict__ rows_sorted, int32_t* __restrict__ n_valid_out,
    float* __restrict__ cost_out, float* cost /* LDS [N][MAXL] (MANY: [2][N][MAXL], the second half holds the IoUs) */,
    float focal_alpha = 0.25f, int64_t* __restrict__ many_rows = nullptr, int64_t* __restrict__ many_cols = nullptr,
    int32_t* __restrict__ many_n = nullptr, int* sorted_lds = nullptr)
{
    __shared__ float t_x[MAXL][256];                 // target xs (S <= 250)
    __shared__ float t_hd[MAXL][3];                  // start y, start x, angle of the label rows (columns 2..4)
    __shared__ float red[4 * QUAD][3];
    __shared__ int t_valid[MAXL], top_rows[MAXL][MAXL], best_combo;
    __shared__ float combo_cost[NT];
    __shared__ unsigned char gone[NT];               // MANY: rows retired by earlier rounds
    __shared__ int ks[MAXL], comp[MAXL], many_count, more;
    const int tid = threadIdx.x;
    const int W = 6 + S;
    if (tid < NT) gone[tid] = 0;

    // label rows -> LDS (the callers' loads of `pred` are in flight meanwhile)
    auto stage = [&]() {
        if (tid < MAXL) t_valid[tid] = (tid < L) && (tgt[tid * W + 1] == 1.0f);
        for (int i = tid; i < L * S; i += NT * QUAD) t_x[i / S][i % S] = tgt[(i / S) * W + 6 + (i % S)];
        if (tid >= 64 && tid < 64 + 3 * MAXL) {
            const int j = (tid - 64) / 3, c = (tid - 64) % 3;
            if (j < L) t_hd[j][c] = tgt[j * W + 2 + c];
        }
        __syncthreads();
    };

    // PF = pf.value: float2 loads of the anchor's x row that are held in registers (0: rows longer than 72 columns go in trips of 16
    // columns, rows of odd width one column at a time)
    auto cost_phase = [&](auto pf) {
    constexpr int PF = decltype(pf)::value;
    if constexpr (QUAD == 4) {
        // ---- one thread per (anchor, label): the label index is wave-uniform ------------------------------------------
        const int a = tid & (NT - 1), jq = tid / NT;
        const bool arow = a < N;
        const float* p = pred + (size_t)(arow ? a : 0) * W;
        const float p1 = p[1], p2 = p[2], p3 = p[3], p4 = p[4];
        float2 xb[PF > 0 ? PF : 1];
        if constexpr (PF > 0) {
#pragma unroll
            for (int u = 0; u < PF; ++u) xb[u] = *reinterpret_cast<const float2*>(p + 6 + (2 * u + 1 < S ? 2 * u : 0));
        }
        stage();
        const bool lab = jq < L && t_valid[jq], on = arow && lab;
        const float tl = lab ? wave_len(t_x[jq], S, img_w) : 0.f;
        float cls = 0.f, dist = 0.f, start = 0.f, theta = 0.f, iou = 0.f;
        float mx_d = -INFINITY, mx_s = -INFINITY, mx_t = -INFINITY;
        if (arow) {
            const float pr = 1.0f / (1.0f + expf(-p1));
            const float negc = -logf(1.0f - pr + 1e-12f) * (1.0f - focal_alpha) * (pr * pr);
            const float posc = -logf(pr + 1e-12f) * focal_alpha * ((1.0f - pr) * (1.0f - pr));
            cls = posc - negc;
        }
        if (on) {
            float d = 0.f, ovr = 0.f, uni = 0.f;
            const float* tx = t_x[jq];
            auto term = [&](int k, float xr) {
                const float x = xr * (img_w - 1.0f), t = tx[k];
                const bool ok = !(t < 0.f) && !(t >= img_w);
                d += ok ? fabsf(t - x) : 0.f;
                ovr += ok ? fminf(x + 15.f, t + 15.f) - fmaxf(x - 15.f, t - 15.f) : 0.f;
                uni += ok ? fmaxf(x + 15.f, t + 15.f) - fminf(x - 15.f, t - 15.f) : 0.f;
            };
            if constexpr (PF > 0) {
#pragma unroll
                for (int u = 0; u < PF; ++u)
                    if (2 * u + 1 < S) { term(2 * u, xb[u].x); term(2 * u + 1, xb[u].y); }
            } else {
                int k = 0;
                if ((W & 1) == 0) {
                    for (; k + 1 < S; k += 16) {
                        float2 buf[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const int kk = k + 2 * u;
                            buf[u] = *reinterpret_cast<const float2*>(p + 6 + (kk + 1 < S ? kk : 0));
                        }
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const int kk = k + 2 * u;
                            if (kk + 1 < S) { term(kk, buf[u].x); term(kk + 1, buf[u].y); }
                        }
                    }
                    k = S & ~1;
                }
                for (; k < S; ++k) term(k, p[6 + k]);
            }
            dist = d / (tl + 1e-9f);
            iou = ovr / (uni + 1e-9f);
            const float* tr = t_hd[jq];
            const float dy = p2 * (img_h - 1.0f) - tr[0] * (img_h - 1.0f), dx = p3 * (img_w - 1.0f) - tr[1] * (img_w - 1.0f);
            start = sqrtf(dy * dy + dx * dx);
            theta = fabsf(p4 - tr[2]) * 180.f;
            mx_d = dist; mx_s = start; mx_t = theta;
        }
        block_max3<16>(mx_d, mx_s, mx_t, red);
        if (arow) {
            float c = INFINITY;
            if (on) {
                const float a_ = 1.0f - dist / (mx_d + 1e-4f);
                const float b_ = 1.0f - start / (mx_s + 1e-4f);
                const float t_ = 1.0f - theta / (mx_t + 1e-4f);
                const float prod = a_ * b_ * t_;
                c = -(prod * prod) * 3.0f + cls - iou;
            }
            cost[a * MAXL + jq] = c;
            if (MANY) cost[(N + a) * MAXL + jq] = on ? fmaxf(iou, 0.f) : -1.f;
            if (cost_out && jq < L) cost_out[(size_t)a * L + jq] = c;
        }
    } else {
    // ---- per-anchor raw terms ------------------------------------------------------------------------------
    float dist[MAXL], start[MAXL], theta[MAXL], iou[MAXL], cls = 0.f;
    float mx_d = -INFINITY, mx_s = -INFINITY, mx_t = -INFINITY;
    const bool arow = tid < N;
    const float* p = pred + (size_t)(arow ? tid : 0) * W;
    const float p1 = p[1], p2 = p[2], p3 = p[3], p4 = p[4];
    float2 xb[PF > 0 ? PF : 1];
    if constexpr (PF > 0) {
#pragma unroll
        for (int u = 0; u < PF; ++u) xb[u] = *reinterpret_cast<const float2*>(p + 6 + (2 * u + 1 < S ? 2 * u : 0));
    }
    stage();
    float tl[MAXL];
#pragma unroll
    for (int j = 0; j < MAXL; ++j) tl[j] = (j < L && t_valid[j]) ? wave_len(t_x[j], S, img_w) : 0.f;
    if (arow) {
        // focal cost of the positive class (focal_cost: alpha .25, gamma 2, eps 1e-12), label column 1
        const float pr = 1.0f / (1.0f + expf(-p1));
        const float negc = -logf(1.0f - pr + 1e-12f) * (1.0f - focal_alpha) * (pr * pr);
        const float posc = -logf(pr + 1e-12f) * focal_alpha * ((1.0f - pr) * (1.0f - pr));
        cls = posc - negc;
        const float psy = p2 * (img_h - 1.0f), psx = p3 * (img_w - 1.0f), pth = p4;
        // one pass over the anchor's S x-columns for all label columns at once (each x is read once, as a float2: the row
        // starts at an even element) - the four per-column sums keep their ascending-k order
        float d[MAXL], ovr[MAXL], uni[MAXL];
#pragma unroll
        for (int j = 0; j < MAXL; ++j) d[j] = ovr[j] = uni[j] = 0.f;
        // branch-free: a branch on the freshly read label value (or on the LDS validity flag) makes every one of the 4 S trips wait
        // for its LDS read - the loop then is a chain of ~150 LDS latencies, most of this kernel's time; adding 0 leaves a sum as it is
        bool col_on[MAXL];
#pragma unroll
        for (int j = 0; j < MAXL; ++j) col_on[j] = j < L && t_valid[j];
        auto term = [&](int k, float xr) {
            const float x = xr * (img_w - 1.0f);
#pragma unroll
            for (int j = 0; j < MAXL; ++j) {
                const float t = t_x[j][k];
                const bool ok = col_on[j] && !(t < 0.f) && !(t >= img_w);
                d[j] += ok ? fabsf(t - x) : 0.f;
                ovr[j] += ok ? fminf(x + 15.f, t + 15.f) - fmaxf(x - 15.f, t - 15.f) : 0.f;
                uni[j] += ok ? fmaxf(x + 15.f, t + 15.f) - fminf(x - 15.f, t - 15.f) : 0.f;
            }
        };
        if constexpr (PF > 0) {
#pragma unroll
            for (int u = 0; u < PF; ++u)
                if (2 * u + 1 < S) { term(2 * u, xb[u].x); term(2 * u + 1, xb[u].y); }
        } else {
            int k = 0;
            if ((W & 1) == 0)
                // 16 columns per trip, their 8 loads issued together (clamped addresses, branch-free): with one load per trip the loop
                // was a chain of S/2 memory latencies (18 x ~0.5 us at S = 36 - most of this kernel's 26 us)
                for (; k + 1 < S; k += 16) {
                    float2 buf[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int kk = k + 2 * u;
                        buf[u] = *reinterpret_cast<const float2*>(p + 6 + (kk + 1 < S ? kk : 0));
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int kk = k + 2 * u;
                        if (kk + 1 < S) { term(kk, buf[u].x); term(kk + 1, buf[u].y); }
                    }
                }
            k = ((W & 1) == 0) ? (S & ~1) : 0;
            for (; k < S; ++k) term(k, p[6 + k]);
        }
#pragma unroll
        for (int j = 0; j < MAXL; ++j) {
            dist[j] = start[j] = theta[j] = iou[j] = 0.f;
            if (j >= L || !t_valid[j]) continue;
            dist[j] = d[j] / (tl[j] + 1e-9f);
            iou[j] = ovr[j] / (uni[j] + 1e-9f);
            const float* tr = t_hd[j];
            const float dy = psy - tr[0] * (img_h - 1.0f), dx = psx - tr[1] * (img_w - 1.0f);
            start[j] = sqrtf(dy * dy + dx * dx);
            theta[j] = fabsf(pth - tr[2]) * 180.f;
            mx_d = fmaxf(mx_d, dist[j]); mx_s = fmaxf(mx_s, start[j]); mx_t = fmaxf(mx_t, theta[j]);
        }
    }
    block_max3<4>(mx_d, mx_s, mx_t, red);
    if (arow) {
#pragma unroll
        for (int j = 0; j < MAXL; ++j) {
            float c = INFINITY;
            if (j < L && t_valid[j]) {
                const float a = 1.0f - dist[j] / (mx_d + 1e-4f);
                const float b = 1.0f - start[j] / (mx_s + 1e-4f);
                const float t = 1.0f - theta[j] / (mx_t + 1e-4f);
                const float prod = a * b * t;
                c = -(prod * prod) * 3.0f + cls - iou[j];
            }
            cost[tid * MAXL + j] = c;
            if (MANY) cost[(N + tid) * MAXL + j] = (j < L && t_valid[j]) ? fmaxf(iou[j], 0.f) : -1.f;
            if (cost_out && j < L) cost_out[(size_t)tid * L + j] = c;
        }
    }
    }
    };
    if ((W & 1) == 0 && S <= 36) cost_phase(PfTag<18>{});
    else if (MAXPF >= 36 && (W & 1) == 0 && S <= 72) cost_phase(PfTag<(MAXPF >= 36 ? 36 : 0)>{});
    else cost_phase(PfTag<0>{});
    __syncthreads();

    if (MANY) {
        // k_j per valid label (compact order = ascending j): the 4 largest clamped IoUs of the column, summed in descending order.
        // A lane reads its CAND candidates once; the rounds run on registers and DPP moves
        const int j = tid >> 6, lane = tid & 63;
        if (j < MAXL) {
            const bool valid = j < L && t_valid[j];
            float cv[CAND]; bool ex[CAND];
#pragma unroll
            for (int q = 0; q < CAND; ++q) {
                const int i = lane + 64 * q;
                ex[q] = !valid || i >= N;
                cv[q] = ex[q] ? 0.f : cost[(N + i) * MAXL + j];
            }
            float sum = 0.f;
#pragma unroll
            for (int r = 0; r < MAXL; ++r) {
                float bv = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
                for (int q = 0; q < CAND; ++q) {
                    const int i = lane + 64 * q;
                    if (!ex[q] && (cv[q] > bv || (cv[q] == bv && i < bi))) { bv = cv[q]; bi = i; }
                }
                wave_arg_best<false>(bv, bi);
#pragma unroll
                for (int q = 0; q < CAND; ++q) ex[q] = ex[q] || (bi == lane + 64 * q);
                if (valid && bi != 0x7fffffff) sum += bv;
            }
            if (lane == 0) {
                const int k = (int)sum;
                ks[j] = valid ? (k < 1 ? 1 : k) : 0;
            }
        }
        if (tid == 0) many_count = 0;
        __syncthreads();
        if (tid == 0) {
            int c = 0;
            for (int j = 0; j < MAXL; ++j) { comp[j] = c; c += (j < L && t_valid[j]); }
            // ks in COMPACT order (the reference filters the valid labels first)
            int kc[MAXL] = {0, 0, 0, 0};
            for (int j = 0; j < MAXL; ++j) if (j < L && t_valid[j]) kc[comp[j]] = ks[j];
            for (int j = 0; j < MAXL; ++j) ks[j] = kc[j];
            more = (kc[0] + kc[1] + kc[2] + kc[3]) > 0;
        }
        __syncthreads();
    }
    for (int round = 0; round < (MANY ? MAXL + 1 : 1); ++round) {
    if (MANY && !more) break;
    // ---- the MAXL cheapest rows of every valid column (wave j <-> column j) -----------------------------------
    // lexicographic (cost, index): a NaN cost is never picked, infinite costs tie by the lowest index, 0x7fffffff = nothing left.
    // A lane reads its CAND candidates and their `gone` flags once; the MAXL rounds run on registers and DPP moves
    {
        const int j = tid >> 6, lane = tid & 63;
        if (j < MAXL) {
            const bool valid = j < L && t_valid[j];
            float cv[CAND]; bool ex[CAND];
#pragma unroll
            for (int q = 0; q < CAND; ++q) {
                const int i = lane + 64 * q;                                  // < NT
                ex[q] = !valid || i >= N || gone[i] != 0;
                cv[q] = ex[q] ? 0.f : cost[i * MAXL + j];
            }
#pragma unroll
            for (int r = 0; r < MAXL; ++r) {
                float bv = INFINITY; int bi = 0x7fffffff;
#pragma unroll
                for (int q = 0; q < CAND; ++q) {
                    const int i = lane + 64 * q;
                    if (!ex[q] && (cv[q] < bv || (cv[q] == bv && i < bi))) { bv = cv[q]; bi = i; }
                }
                wave_arg_best<true>(bv, bi);
#pragma unroll
                for (int q = 0; q < CAND; ++q) ex[q] = ex[q] || (bi == lane + 64 * q);
                if (lane == 0) top_rows[j][r] = valid ? bi : -1;
            }
        }
    }
    __syncthreads();

    // ---- enumerate candidate combinations: thread t <-> (t&3, (t>>2)&3, (t>>4)&3, t>>6) -----------------------
    {
        int rows[MAXL];
        float total = 0.f;
        bool ok = true;
#pragma unroll
        for (int j = 0; j < MAXL; ++j) {
            const int pick = (tid >> (2 * j)) & 3;
            const bool valid = j < L && t_valid[j];
            rows[j] = valid ? top_rows[j][pick] : -1;
            if (!valid) { ok = ok && pick == 0; continue; }          // one representative per invalid column
            if (rows[j] < 0 || rows[j] == 0x7fffffff) { ok = false; continue; }
            total += cost[rows[j] * MAXL + j];
#pragma unroll
            for (int q = 0; q < j; ++q) ok = ok && !(rows[q] >= 0 && rows[q] == rows[j]);
        }
        if (tid < NT) combo_cost[tid] = ok ? total : INFINITY;
    }
    __syncthreads();
    if (tid < 64) {
        float bv = INFINITY; int bi = 0x7fffffff;
        for (int c = tid; c < NT; c += 64) {
            const float v = combo_cost[c];
            if (v < bv || (v == bv && c < bi)) { bv = v; bi = c; }
        }
        wave_arg_best<true>(bv, bi);
        // every combination invalid (fewer free anchors than valid label rows): no match at all, not combination 0, whose
        // columns would share an anchor.  With no valid label, combination 0 is valid and costs 0.
        if (tid == 0) best_combo = bv < INFINITY ? bi : 0x7fffffff;
    }
    __syncthreads();
    if (tid == 0) {
        int rows[MAXL], nv = 0;
        for (int j = 0; j < MAXL; ++j) {
            const bool valid = j < L && t_valid[j];
            rows[j] = (valid && best_combo != 0x7fffffff) ? top_rows[j][(best_combo >> (2 * j)) & 3] : -1;
            if (j < L && rows_by_col) rows_by_col[j] = rows[j];
            nv += rows[j] >= 0;
        }
        // ascending valid rows first (prior-index order, as scipy returns them), then -1
        for (int a = 0; a < MAXL; ++a)
            for (int b = a + 1; b < MAXL; ++b) {
                const bool swap = (rows[b] >= 0) && (rows[a] < 0 || rows[b] < rows[a]);
                if (swap) { const int t = rows[a]; rows[a] = rows[b]; rows[b] = t; }
            }
        if (!MANY) {
            for (int j = 0; j < L; ++j) rows_sorted[j] = rows[j];
            if (sorted_lds)
                for (int j = 0; j < MAXL; ++j) sorted_lds[j] = rows[j];
            if (n_valid_out) *n_valid_out = nv;
        } else {
            // pairs in row-sorted order: position p carries (row, label); keep where k_p > 0, retire the kept rows
            int lab[MAXL];
            for (int p_ = 0; p_ < MAXL; ++p_) {
                lab[p_] = -1;
                if (rows[p_] < 0) continue;
                for (int j = 0; j < MAXL; ++j)
                    if (j < L && t_valid[j] && best_combo != 0x7fffffff && top_rows[j][(best_combo >> (2 * j)) & 3] == rows[p_]) lab[p_] = j;
            }
            for (int p_ = 0; p_ < MAXL; ++p_) {
                if (rows[p_] < 0 || ks[p_] <= 0) continue;
                many_rows[many_count] = rows[p_];
                many_cols[many_count] = lab[p_];
                ++many_count;
                gone[rows[p_]] = 1;
            }
            int any = 0;
            for (int j = 0; j < MAXL; ++j) { if (ks[j] > 0) --ks[j]; any += ks[j]; }
            more = any > 0 && nv > 0;
        }
    }
    __syncthreads();
    }   // rounds
    if (MANY && tid == 0) {
        for (int i = many_count; i < MAXL * MAXL; ++i) { many_rows[i] = -1; many_cols[i] = -1; }
        if (many_n) *many_n = many_count;
    }
}


}  // namespace phassign
