// Training targets on the device: the annotated lane points of F frames -> the [R][6+S] label rows of the reference's
// libs/dataset/openlane/transforms.py (transform_annotation, filter_lane, sample_lane; datasetOL.py:47-59 for crop and flip), in
// one launch (DESIGN.md "Training targets").  Arithmetic: float64 throughout, the float32 input points widened exactly, one cast to
// float32 at the end; nothing is contracted.
//
// Rules, per frame (S offsets, R rows, strip_size = img_h / (S - 1), ys = the caller's offsets_ys table, strictly descending):
//   0. map, per point:  y = y - crop;  flip: x = (src_w - 1) - x;  x = x * scale_x;  y = y * scale_y.
//   0b. (phnet_lane_targets_aug only; the label half of csrc/augment.hip) in output pixels:  flip2[f]: x = (img_w - 1) - x;  then
//      (x, y) = ((f00 x + f01 y) + f02, (f10 x + f11 y) + f12) with f = fwd[f], the source -> output matrix.  A null array skips its step.
//   0c. (phnet_lane_targets_clip with clip = 1 only) clip to the rectangle 0 <= x <= Wc = img_w - 1e-3, 0 <= y <= Hc = img_h - 1e-3, on
//      the mapped points in input order.  A lane with a non-finite mapped coordinate is ONE fragment with all its points.  Else
//      every maximal run p_a .. p_b of points inside gives the fragment [E] p_a .. p_b [X]: E (iff a > 0) the crossing of
//      p_a -> p_(a-1), X (iff b < n - 1) the crossing of p_b -> p_(b+1).  Crossing from q (in) towards o (out): for each coordinate c
//      whose bound (0, Wc or Hc) o violates t_c = (bound - q_c) / (o_c - q_c); t the smaller; the point q + t * (o - q) with the
//      coordinate(s) that gave t set to the bound itself (a tie: both, a corner); a crossing equal to q is dropped.  A segment
//      with both ends outside produces nothing, even where it crosses the image (its two-point fragment would fall to rule 1).
//   1. filter:  lanes l < clamp(lanes_num, 0, Lin) with clamp(count, 0, P) > 2 points survive and are numbered in order; lane
//      number r owns output row r, numbers >= R are ignored, rows without a lane get the default row.  With rule 0c the same on
//      fragments: those of more than 2 points survive, numbered in order of (input lane, run).
//   2. default row:  [0] = 1, [1] = 0, everything else -1e5.  A lane with a non-finite mapped coordinate leaves it.
//   3. sort stably by descending y; of equal y only the first in input order stays; then x = (x * img_w) / img_w and
//      y = (y * img_h) / img_h.  n points remain; n < 2 leaves the default row.
//   4. interpolant over ascending y (t_i, v_i):  n = 2 the line v0 + (y - t0) * ((v1 - v0) / (t1 - t0));  n = 3 the parabola in
//      Newton form v0 + (y - t0) * (d01 + (y - t1) * d012);  n >= 4 the not-a-knot cubic spline: knot derivatives s_i from the
//      tridiagonal system (forward elimination without pivoting, back substitution), and in the interval t_i <= y <= t_(i+1)
//      (binary search, i <= n - 2)  h = t_(i+1) - t_i, m = (v_(i+1) - v_i) / h, tt = (s_i + s_(i+1) - 2 m) / h, c0 = tt / h,
//      c1 = (m - s_i) / h - tt, d = y - t_i, x = ((c0 d + c1) d + s_i) d + v_i.
//   5. sample, table order:  ys > y_max: the line through the two bottom-most points, v_(n-1) + (ys - t_(n-1)) * slope;
//      y_min <= ys <= y_max: the interpolant; ys < y_min: dropped.  No row of the second kind leaves the default row.
//   6. a value is inside iff 0 <= x < img_w; all outside values come first, then the inside ones, each group in table order
//      (outside values in the middle or at the top of a lane move to the front: the reference's quirk, kept).
//   7. n_in <= 1 leaves the default row.  Else [0] = 0, [1] = 1, [2] = n_out / (S - 1), [3] = inside[0] / (img_w - 1), [4] = the
//      mean over i = 1 .. n_in - 1 of t_i = atan(i * strip_size / (inside[i] - inside[0] + 1e-5)) / pi, with 1 - |t_i| where
//      not t_i > 0, summed in ascending i; [5] = n_in / (S - 1); [6 ..] = the reordered values, then -1e5.
//
// One workgroup of ONE wavefront per (frame, output row).  A ballot over the <= 64 counts finds the wave's lane; the points are
// mapped into LDS, rank-sorted there (each lane counts the points above its own) with the duplicates compacted in the same pass;
// lane 0 runs the serial tridiagonal solve on LDS arrays; the 64 lanes then take the S sample rows in strides, and ballots with
// prefix counts place the values.  Lane 0 sums the thetas in order.  Every branch on data is wave-uniform; no atomics, plain
// vector stores, every element of the row is written exactly once.
// Rule 0c, in the same wavefront: it walks the frame's lanes 64 points at a time; each lane decides from its point and three neighbours
// whether a surviving run ENDS at its point (a run of 1 or 2 points survives by its crossings, a longer one always), so one ballot per
// 64 points counts the fragments and no state crosses from one ballot to the next.  The wave of row r stops at the lane that holds
// fragment r, finds the run's two ends from the ballots of that lane (k-th set bit; the highest outside point below it) and stages
// [E] p_a .. p_b [X] where the unclipped path stages the whole lane.  The wave of row 0 walks every lane and writes frag_count.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxInLanes = 64;               // Lin: one ballot over the counts
constexpr int kMaxPoints = 256;               // P
constexpr int kMaxRows = 64;                  // R
constexpr int kMaxOffsets = 256;              // S
constexpr int kMaxGridX = 65536;              // frames beyond this are walked by the same workgroups
constexpr float kInvalid = -1e5f;
constexpr double kPi = 3.141592653589793;
constexpr double kDblMax = 1.7976931348623157e308;

struct LaneMap { double crop, src_w, scale_x, scale_y; int flip; const int* flip2; const double* fwd; int clip; int* frag_count; };
// flip2, fwd: rule 0b, or null.  clip: rule 0c.  frag_count [F] or null: the frame's surviving fragments (lanes without rule 0c)
struct Pt { double x, y; };

__device__ __forceinline__ void write_default(float* __restrict__ row, int W, int lane) {
#pragma unroll 1
    for (int k = lane; k < W; k += 64) row[k] = k == 0 ? 1.0f : (k == 1 ? 0.0f : kInvalid);
}

// rule 4, n >= 4: the knot derivatives into s[], by one lane.  cp[] is scratch.
__device__ __forceinline__ void knot_derivatives(const double* t, const double* v, double* cp, double* s, int n) {
#pragma clang fp contract(off)
    const double h0 = t[1] - t[0], h1 = t[2] - t[1], d0 = t[2] - t[0];
    const double m0 = (v[1] - v[0]) / h0, m1 = (v[2] - v[1]) / h1;
    cp[0] = d0 / h1;
    s[0] = (((h0 + 2.0 * d0) * h1) * m0 + (h0 * h0) * m1) / d0 / h1;
    double hp = h0, mprev = m0;                                                    // h_(i-1), m_(i-1)
#pragma unroll 1
    for (int i = 1; i < n - 1; ++i) {
        const double hi = t[i + 1] - t[i], mi = (v[i + 1] - v[i]) / hi;
        const double den = 2.0 * (hp + hi) - hi * cp[i - 1];
        cp[i] = hp / den;
        s[i] = (3.0 * (hi * mprev + hp * mi) - hi * s[i - 1]) / den;
        hp = hi; mprev = mi;
    }
    // hp = h_(n-2), mprev = m_(n-2)
    const double hq = t[n - 2] - t[n - 3], mq = (v[n - 2] - v[n - 3]) / hq;      // h_(n-3), m_(n-3)
    const double d1 = t[n - 1] - t[n - 3];
    const double den = hq - d1 * cp[n - 2];
    const double rhs = ((hp * hp) * mq + ((2.0 * d1 + hp) * hq) * mprev) / d1;
    s[n - 1] = (rhs - d1 * s[n - 2]) / den;
#pragma unroll 1
    for (int i = n - 2; i >= 0; --i) s[i] = s[i] - cp[i] * s[i + 1];
}

// rule 4 at y, t[0] <= y <= t[n-1]
__device__ __forceinline__ double interpolate(const double* t, const double* v, const double* s, int n, double y) {
#pragma clang fp contract(off)
    if (n == 2) return v[0] + (y - t[0]) * ((v[1] - v[0]) / (t[1] - t[0]));
    if (n == 3) {
        const double d01 = (v[1] - v[0]) / (t[1] - t[0]);
        const double d12 = (v[2] - v[1]) / (t[2] - t[1]);
        const double d012 = (d12 - d01) / (t[2] - t[0]);
        return v[0] + (y - t[0]) * (d01 + (y - t[1]) * d012);
    }
    int lo = 0, hi = n - 2;                                                        // the last i with t[i] <= y, at most n - 2
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t[mid] <= y) lo = mid; else hi = mid - 1;
    }
    const double h = t[lo + 1] - t[lo];
    const double m = (v[lo + 1] - v[lo]) / h;
    const double tt = (s[lo] + s[lo + 1] - 2.0 * m) / h;
    const double c0 = tt / h;
    const double c1 = (m - s[lo]) / h - tt;
    const double d = y - t[lo];
    return ((c0 * d + c1) * d + s[lo]) * d + v[lo];
}

__device__ __forceinline__ bool is_inside(double x, double img_w) { return x >= 0.0 && x < img_w; }             // false for NaN

// rules 0 and 0b on point i of a lane (m: the frame's matrix; flip2 and fwd select per lane, see encode_row)
__device__ __forceinline__ Pt map_point(const float* __restrict__ lp, int i, const LaneMap& mp, int flip2, const double* m, double img_w) {
#pragma clang fp contract(off)
    double x = (double)lp[2 * i], y = (double)lp[2 * i + 1];
    y = y - mp.crop;
    if (mp.flip) x = (mp.src_w - 1.0) - x;
    x = x * mp.scale_x;
    y = y * mp.scale_y;
    x = flip2 ? (img_w - 1.0) - x : x;
    const double xa = (m[0] * x + m[1] * y) + m[2], ya = (m[3] * x + m[4] * y) + m[5];
    x = mp.fwd ? xa : x;
    y = mp.fwd ? ya : y;
    return Pt{x, y};
}

__device__ __forceinline__ bool is_finite(Pt p) { return fabs(p.x) <= kDblMax && fabs(p.y) <= kDblMax; }         // false for NaN, +-inf
__device__ __forceinline__ bool in_rect(Pt p, double Wc, double Hc) { return p.x >= 0.0 && p.x <= Wc && p.y >= 0.0 && p.y <= Hc; }

// rule 0c: the crossing from q (in) towards o (out) into c; false: it equals q and is dropped.  Plain arithmetic on any input.
__device__ __forceinline__ bool crossing(Pt q, Pt o, double Wc, double Hc, Pt& c) {
#pragma clang fp contract(off)
    const bool vx = o.x < 0.0 || o.x > Wc, vy = o.y < 0.0 || o.y > Hc;
    const double bx = o.x < 0.0 ? 0.0 : Wc, by = o.y < 0.0 ? 0.0 : Hc;
    const double tx = (bx - q.x) / (o.x - q.x), ty = (by - q.y) / (o.y - q.y);
    const bool use_x = vx && (!vy || tx <= ty), use_y = vy && (!vx || ty <= tx);
    const double t = use_x ? tx : ty;
    const double x = q.x + t * (o.x - q.x), y = q.y + t * (o.y - q.y);
    c.x = use_x ? bx : x;
    c.y = use_y ? by : y;
    return !(c.x == q.x && c.y == q.y);
}

// rule 0c on points base .. base + 63 of a finite lane of n points: ends = the points at which a surviving run ends, outs = the
// points outside, bads = the non-finite ones (then the other two mean nothing)
__device__ __forceinline__ void clip_ballots(const float* __restrict__ lp, int n, int base, int lane, const LaneMap& mp, int flip2,
                                             const double* m, double img_w, double Wc, double Hc, unsigned long long& ends,
                                             unsigned long long& outs, unsigned long long& bads) {
    const int i = base + lane, i0 = min(i, n - 1);
    const bool valid = i < n;
    const Pt p = map_point(lp, i0, mp, flip2, m, img_w), pm1 = map_point(lp, max(i0 - 1, 0), mp, flip2, m, img_w);
    const Pt pm2 = map_point(lp, max(i0 - 2, 0), mp, flip2, m, img_w), pp1 = map_point(lp, min(i0 + 1, n - 1), mp, flip2, m, img_w);
    // the flags are 0 / 1 integers held in vector registers: as wave masks a dozen of them at once would not fit the scalar file
    int in0 = in_rect(p, Wc, Hc), in1 = (i0 >= 1) & in_rect(pm1, Wc, Hc), in2 = (i0 >= 2) & in_rect(pm2, Wc, Hc);
    int inn = (i0 < n - 1) & in_rect(pp1, Wc, Hc);
    asm volatile("" : "+v"(in0), "+v"(in1), "+v"(in2), "+v"(inn));
    Pt c;
    int x0 = crossing(p, pp1, Wc, Hc, c);                                          // the run that ends here has its X
    asm volatile("" : "+v"(x0));
    int e0 = crossing(p, pm1, Wc, Hc, c);                                          // a run that starts here has its E
    asm volatile("" : "+v"(e0));
    int e1 = crossing(pm1, pm2, Wc, Hc, c);                                        // a run that starts one point earlier has its E
    asm volatile("" : "+v"(e1));
    x0 &= (i0 < n - 1) & (inn ^ 1);
    e0 &= (i0 >= 1) & (in1 ^ 1);
    e1 &= (i0 >= 2) & (in2 ^ 1);
    const int end = (int)valid & in0 & (inn ^ 1);
    const int sv = end & ((in1 & in2) | (in1 & (in2 ^ 1) & (e1 | x0)) | ((in1 ^ 1) & e0 & x0));      // runs of >= 3, of 2, of 1 points
    ends = __ballot(sv);
    outs = __ballot((int)valid & (in0 ^ 1));
    bads = __ballot(valid & !is_finite(p));
}

struct Lds {
    double a[kMaxPoints];                     // mapped x of the input points; then the sampled values in table order
    double b[kMaxPoints];                     // mapped y of the input points; then the reordered values
    double t[kMaxPoints], v[kMaxPoints];      // rule 3: ascending y and its x
    double cp[kMaxPoints];                    // elimination scratch; then the thetas
    double s[kMaxPoints];                     // knot derivatives
    int first[kMaxPoints];                    // 1: no earlier input point has this y
};

__device__ __forceinline__ void encode_row(Lds& L, const float* __restrict__ points, const int* __restrict__ counts,
                                           const int* __restrict__ lanes_num, const double* __restrict__ ys_tab,
                                           float* __restrict__ row, size_t f, int r, int Lin, int P, int S, double img_h, double img_w,
                                           double strip, const LaneMap& mp, int lane)
{
#pragma clang fp contract(off)
    const int W = 6 + S;
    const unsigned long long below = (1ull << lane) - 1ull;

    const int nl = min(max(lanes_num[f], 0), Lin);
    int cnt = 0;
    if (lane < nl) cnt = min(max(counts[f * Lin + lane], 0), P);
    // rule 0b: the frame's matrix goes through lanes 0-5 into vector registers (as scalars its twelve words would not fit beside the
    // arguments); the pointers are vector values (see the kernel), so the two steps are per-lane selects, not branches
    const int flip2 = mp.flip2 ? mp.flip2[f] : 0;
    double m[6];
    {
        const double mine = mp.fwd ? mp.fwd[f * 6 + (size_t)min(lane, 5)] : 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) m[k] = __shfl(mine, k, 64);
    }
    int n_raw;
    bool bad = false;
    if (!mp.clip) {
        // ---- rule 1: the r-th surviving lane of the frame ----
        unsigned long long surv = __ballot(cnt > 2);
        if (r == 0 && lane == 0 && mp.frag_count) mp.frag_count[f] = __builtin_popcountll(surv);
        for (int k = 0; k < r && surv; ++k) surv &= surv - 1ull;
        if (!surv) { write_default(row, W, lane); return; }
        const int lsel = __builtin_ctzll(surv);
        n_raw = __builtin_amdgcn_readfirstlane(__shfl(cnt, lsel, 64));             // 3 .. P

        // ---- rule 0 into LDS; rule 2 ----
        const float* lp = points + ((f * Lin + lsel) * P) * 2;
#pragma unroll 1
        for (int i = lane; i < n_raw; i += 64) {
            const Pt p = map_point(lp, i, mp, flip2, m, img_w);
            bad |= !is_finite(p);
            L.a[i] = p.x; L.b[i] = p.y;
        }
    } else {
        // ---- rules 0c and 1: the r-th surviving fragment of the frame ----
        const double Wc = img_w - 1e-3, Hc = img_h - 1e-3;
        int seen = 0, lsel = -1, k_sel = 0, sel_bad = 0;
#pragma unroll 1
        for (int l = 0; l < nl; ++l) {
            const int n = __builtin_amdgcn_readfirstlane(__shfl(cnt, l, 64));
            if (n <= 2) continue;                                                  // at most [p, X] or [E, p]: never more than 2 points
            const float* lp = points + ((f * Lin + l) * P) * 2;
            int c = 0, lane_bad = 0;
#pragma unroll 1
            for (int base = 0; base < n; base += 64) {
                unsigned long long ends, outs, bads;
                clip_ballots(lp, n, base, lane, mp, flip2, m, img_w, Wc, Hc, ends, outs, bads);
                c += __builtin_popcountll(ends);
                lane_bad |= bads != 0ull;
            }
            if (lane_bad) c = 1;                                                   // one fragment, all its points
            if (lsel < 0 && r < seen + c) { lsel = l; k_sel = r - seen; sel_bad = lane_bad; }
            seen += c;
            if (lsel >= 0 && r != 0) break;                                        // row 0 goes on: it counts the frame
        }
        if (r == 0 && lane == 0 && mp.frag_count) mp.frag_count[f] = seen;
        if (lsel < 0 || sel_bad) { write_default(row, W, lane); return; }          // no fragment; rule 2

        // the run a .. b of fragment k_sel of lane lsel
        const int n = __builtin_amdgcn_readfirstlane(__shfl(cnt, lsel, 64));
        const float* lp = points + ((f * Lin + lsel) * P) * 2;
        int a = 0, b = -1, last_out = -1;
#pragma unroll 1
        for (int base = 0; base < n && b < 0; base += 64) {
            unsigned long long ends, outs, bads;
            clip_ballots(lp, n, base, lane, mp, flip2, m, img_w, Wc, Hc, ends, outs, bads);
            const int pc = __builtin_popcountll(ends);
            if (k_sel < pc) {
                for (int k = 0; k < k_sel; ++k) ends &= ends - 1ull;
                const int bit = __builtin_ctzll(ends);
                b = base + bit;
                outs &= (1ull << bit) - 1ull;
            } else {
                k_sel -= pc;
            }
            if (outs) last_out = base + 63 - __builtin_clzll(outs);
            a = last_out + 1;
        }
        // b >= a >= 0 here: the first pass counted this run.  Every lane computes the two crossings, on the same values
        b = min(max(b, a), n - 1);
        const Pt pa = map_point(lp, a, mp, flip2, m, img_w), pam = map_point(lp, max(a - 1, 0), mp, flip2, m, img_w);
        const Pt pb = map_point(lp, b, mp, flip2, m, img_w), pbp = map_point(lp, min(b + 1, n - 1), mp, flip2, m, img_w);
        Pt ce, cx;
        const bool has_e = (a > 0) & crossing(pa, pam, Wc, Hc, ce), has_x = (b < n - 1) & crossing(pb, pbp, Wc, Hc, cx);
        const int e = __ballot(has_e) != 0ull ? 1 : 0, x = __ballot(has_x) != 0ull ? 1 : 0;
        n_raw = (b - a + 1) + e + x;                                               // 3 .. kMaxPoints (P <= 254 here)
        if (lane == 0 && e) { L.a[0] = ce.x; L.b[0] = ce.y; bad |= !is_finite(ce); }
        if (lane == 0 && x) { L.a[n_raw - 1] = cx.x; L.b[n_raw - 1] = cx.y; bad |= !is_finite(cx); }
#pragma unroll 1
        for (int i = lane; i <= b - a; i += 64) {
            const Pt p = map_point(lp, a + i, mp, flip2, m, img_w);
            L.a[e + i] = p.x; L.b[e + i] = p.y;
        }
    }
    const bool any_bad = __ballot(bad) != 0ull;
    __syncthreads();
    if (any_bad) { write_default(row, W, lane); return; }

    // ---- rule 3: first occurrences, then the rank among them ----
    int n = 0;
#pragma unroll 1
    for (int base = 0; base < n_raw; base += 64) {
        const int i = base + lane;
        bool first = false;
        if (i < n_raw) {
            const double y = L.b[i];
            first = true;
#pragma unroll 1
            for (int j = 0; j < i; ++j) first = first && !(L.b[j] == y);
            L.first[i] = first ? 1 : 0;
        }
        n += __builtin_popcountll(__ballot(first));
    }
    __syncthreads();
#pragma unroll 1
    for (int i = lane; i < n_raw; i += 64) {
        if (!L.first[i]) continue;
        const double y = L.b[i];
        int pos = 0;
#pragma unroll 1
        for (int j = 0; j < n_raw; ++j) pos += (L.first[j] && L.b[j] > y) ? 1 : 0;
        const int asc = n - 1 - pos;                                               // in [0, n): pos counts other first points only
        L.t[asc] = (y * img_h) / img_h;
        L.v[asc] = (L.a[i] * img_w) / img_w;
    }
    __syncthreads();
    if (n < 2) { write_default(row, W, lane); return; }

    // ---- rule 4: the serial solve ----
    if (n >= 4 && lane == 0) knot_derivatives(L.t, L.v, L.cp, L.s, n);
    __syncthreads();

    // ---- rule 5 ----
    const double y_min = L.t[0], y_max = L.t[n - 1], x_bot = L.v[n - 1];
    const double slope = (L.v[n - 1] - L.v[n - 2]) / (L.t[n - 1] - L.t[n - 2]);
    int m_tot = 0, n_ext = 0;
#pragma unroll 1
    for (int base = 0; base < S; base += 64) {
        const int j = base + lane;
        bool keep = false, ext = false;
        double x = 0.0;
        if (j < S) {
            const double y = ys_tab[j];
            if (y > y_max) { keep = ext = true; x = x_bot + (y - y_max) * slope; }
            else if (y >= y_min) { keep = true; x = interpolate(L.t, L.v, L.s, n, y); }
        }
        const unsigned long long kb = __ballot(keep);
        if (keep) L.a[m_tot + __builtin_popcountll(kb & below)] = x;               // < S
        m_tot += __builtin_popcountll(kb);
        n_ext += __builtin_popcountll(__ballot(ext));
    }
    __syncthreads();
    if (m_tot - n_ext <= 0) { write_default(row, W, lane); return; }

    // ---- rule 6 ----
    int n_out = 0;
#pragma unroll 1
    for (int base = 0; base < m_tot; base += 64) {
        const int k = base + lane;
        n_out += __builtin_popcountll(__ballot(k < m_tot && !is_inside(L.a[min(k, m_tot - 1)], img_w)));
    }
    const int n_in = m_tot - n_out;
    if (n_in <= 1) { write_default(row, W, lane); return; }
    int run_in = 0, run_out = 0;
#pragma unroll 1
    for (int base = 0; base < m_tot; base += 64) {
        const int k = base + lane;
        const double x = L.a[min(k, m_tot - 1)];
        const bool in = k < m_tot && is_inside(x, img_w), out = k < m_tot && !in;
        const unsigned long long ib = __ballot(in), ob = __ballot(out);
        if (in) L.b[n_out + run_in + __builtin_popcountll(ib & below)] = x;
        if (out) L.b[run_out + __builtin_popcountll(ob & below)] = x;
        run_in += __builtin_popcountll(ib);
        run_out += __builtin_popcountll(ob);
    }
    __syncthreads();

    // ---- rule 7 ----
    const double x0 = L.b[n_out];
#pragma unroll 1
    for (int i = 1 + lane; i < n_in; i += 64) {
        double th = atan(((double)i * strip) / ((L.b[n_out + i] - x0) + 1e-5)) / kPi;
        if (!(th > 0.0)) th = 1.0 - fabs(th);
        L.cp[i] = th;
    }
    __syncthreads();
    if (lane == 0) {
        double total = 0.0;
#pragma unroll 1
        for (int i = 1; i < n_in; ++i) total = total + L.cp[i];
        row[0] = 0.0f;
        row[1] = 1.0f;
        row[2] = (float)((double)n_out / (double)(S - 1));
        row[3] = (float)(x0 / (img_w - 1.0));
        row[4] = (float)(total / (double)(n_in - 1));
        row[5] = (float)((double)n_in / (double)(S - 1));
    }
#pragma unroll 1
    for (int k = lane; k < S; k += 64) row[6 + k] = k < m_tot ? (float)L.b[k] : kInvalid;
}

__global__ __launch_bounds__(64) void lane_targets_kernel(const float* __restrict__ points, const int* __restrict__ counts,
                                                           const int* __restrict__ lanes_num, const double* __restrict__ ys_tab,
                                                           float* __restrict__ out, long long F, int Lin, int P, int R, int S,
                                                           double img_h, double img_w, double strip, LaneMap mp)
{
    __shared__ Lds L;
    const int lane = threadIdx.x, r = blockIdx.y;
    // the pointers of rules 0b and 0c, the four doubles of rule 0, the image size, the table and the points pointer live in vector
    // registers: held as scalars across the frame loop beside the other arguments and the wave masks of rule 0c they spill (the
    // values and the arithmetic on them are unchanged)
    asm volatile("" : "+v"(mp.flip2), "+v"(mp.fwd), "+v"(mp.crop), "+v"(mp.src_w), "+v"(mp.scale_x), "+v"(mp.scale_y), "+v"(mp.frag_count),
                 "+v"(img_h), "+v"(img_w), "+v"(strip), "+v"(ys_tab), "+v"(points));
#pragma unroll 1
    for (long long f = blockIdx.x; f < F; f += gridDim.x) {
        encode_row(L, points, counts, lanes_num, ys_tab, out + ((size_t)f * R + r) * (size_t)(6 + S), (size_t)f, r, Lin, P, S, img_h,
                   img_w, strip, mp, lane);
        __syncthreads();                                                           // the next frame reuses the LDS arrays
    }
}

static inline bool positive_finite(double v) { return v > 0.0 && v <= kDblMax; }

}  // namespace

// points f32 [F][Lin][P][2] (x, y), counts i32 [F][Lin], lanes_num i32 [F], offsets_ys f64 [S] (device), out f32 [F][R][6+S].
// 1 <= F < 2^31, 1 <= Lin <= 64, 2 <= P <= 256, 1 <= R <= 64, 2 <= S <= 256; img_h, img_w, strip_size, scale_x, scale_y finite
// and > 0, crop and src_w finite, flip 0 or 1, all pointers non-null.  clip 0 or 1, and P <= 254 with clip = 1: a fragment of rule 0c
// has up to P + 2 points and the LDS arrays hold 256.  flip2, fwd and frag_count may be null.
static int launch_lane_targets(const float* points, const int32_t* counts, const int32_t* lanes_num, const double* offsets_ys, float* out,
                               int64_t F, int32_t Lin, int32_t P, int32_t R, int32_t S, double img_h, double img_w, double strip_size,
                               double crop, double src_w, double scale_x, double scale_y, int32_t flip, const int32_t* flip2,
                               const double* fwd, int32_t clip, int32_t* frag_count, void* stream)
{
    if (!points || !counts || !lanes_num || !offsets_ys || !out) return PHNET_ERR_ARG;
    if (F < 1 || F > 0x7fffffffll || Lin < 1 || Lin > kMaxInLanes || P < 2 || P > kMaxPoints || R < 1 || R > kMaxRows || S < 2 ||
        S > kMaxOffsets)
        return PHNET_ERR_ARG;
    if (!positive_finite(img_h) || !positive_finite(img_w) || !positive_finite(strip_size) || !positive_finite(scale_x) ||
        !positive_finite(scale_y))
        return PHNET_ERR_ARG;
    if (!(fabs(crop) <= kDblMax) || !(fabs(src_w) <= kDblMax) || (flip != 0 && flip != 1)) return PHNET_ERR_ARG;
    if ((clip != 0 && clip != 1) || (clip == 1 && P > kMaxPoints - 2)) return PHNET_ERR_ARG;
    const LaneMap mp{crop, src_w, scale_x, scale_y, (int)flip, flip2, fwd, (int)clip, frag_count};
    const unsigned gx = (unsigned)(F < kMaxGridX ? F : kMaxGridX);
    hipLaunchKernelGGL(lane_targets_kernel, dim3(gx, (unsigned)R), dim3(64), 0, (hipStream_t)stream, points, counts, lanes_num,
                       offsets_ys, out, (long long)F, (int)Lin, (int)P, (int)R, (int)S, img_h, img_w, strip_size, mp);
    return phnet_launch_status();
}

PHNET_API int phnet_lane_targets(const float* points, const int32_t* counts, const int32_t* lanes_num, const double* offsets_ys,
                                 float* out, int64_t F, int32_t Lin, int32_t P, int32_t R, int32_t S, double img_h, double img_w,
                                 double strip_size, double crop, double src_w, double scale_x, double scale_y, int32_t flip,
                                 void* stream)
{
    return launch_lane_targets(points, counts, lanes_num, offsets_ys, out, F, Lin, P, R, S, img_h, img_w, strip_size, crop, src_w, scale_x,
                               scale_y, flip, nullptr, nullptr, 0, nullptr, stream);
}

// The same launch with rule 0b: flip2 i32 [F] and fwd f64 [F][6] on the device, each optional (null skips its step; with both null
// this is phnet_lane_targets).  Their values cannot be checked here; a non-finite product leaves the lane's row the default row.
PHNET_API int phnet_lane_targets_aug(const float* points, const int32_t* counts, const int32_t* lanes_num, const double* offsets_ys,
                                     float* out, int64_t F, int32_t Lin, int32_t P, int32_t R, int32_t S, double img_h, double img_w,
                                     double strip_size, double crop, double src_w, double scale_x, double scale_y, int32_t flip,
                                     const int32_t* flip2, const double* fwd, void* stream)
{
    return launch_lane_targets(points, counts, lanes_num, offsets_ys, out, F, Lin, P, R, S, img_h, img_w, strip_size, crop, src_w, scale_x,
                               scale_y, flip, flip2, fwd, 0, nullptr, stream);
}

// The same launch with rule 0c (clip = 1) and the per-frame fragment count: frag_count i32 [F] on the device or null, written on every
// call - the surviving fragments of the frame before the R cap; with clip = 0 the surviving lanes, and out is phnet_lane_targets_aug's.
PHNET_API int phnet_lane_targets_clip(const float* points, const int32_t* counts, const int32_t* lanes_num, const double* offsets_ys,
                                      float* out, int64_t F, int32_t Lin, int32_t P, int32_t R, int32_t S, double img_h, double img_w,
                                      double strip_size, double crop, double src_w, double scale_x, double scale_y, int32_t flip,
                                      const int32_t* flip2, const double* fwd, int32_t clip, int32_t* frag_count, void* stream)
{
    return launch_lane_targets(points, counts, lanes_num, offsets_ys, out, F, Lin, P, R, S, img_h, img_w, strip_size, crop, src_w, scale_x,
                               scale_y, flip, flip2, fwd, clip, frag_count, stream);
}
