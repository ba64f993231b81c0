// Validation F1 on the device (DESIGN.md "Validation F1"): the two steps of the CULane-style evaluator that used to be host
// arithmetic around the mask kernels of lane_iou.hip.  `lane_eval_segments_kernel` turns the polylines of phnet_lane_points and a
// packed annotation table into the evaluator's cv::line segment table (evaluation/culane/src/spline.cpp, lane_compare.cpp:22-49),
// `lane_eval_count_kernel` runs the evaluator's matching and counters (include/hungarianGraph.hpp:39-67, counter.cpp:83-161) on the
// IoU matrices phnet_lane_iou_groups writes.  No host synchronisation, no atomics on floats, every output element written on
// every call.  The host code these restate is phnet_amd/evaluation/culane.py and generate_lane.py.
//
// Segment rules (double arithmetic, nothing contracted into an fma):
//   1. presence.  Annotation g of image f is present iff g < clamp(gt_num[f], 0, G); it has n = clamp(gt_count, 0, P) points.
//      Prediction k is present iff k < clamp(lanes_num[f], 0, L) and, in wire mode, clamp(count, 0, S) > 2 (the len(pts) > 2
//      filter of format_pred_lines); it has n = clamp(count, 0, S) points.  lane_pts = n for a present lane, -1 otherwise.
//   2. wire mode (mode 0; format_pred_lines -> read_lane_file).  Points are taken last to first; vx = (double(tx) * size_w) / 2,
//      vy = (double(ty) * size_h + crop_top) / 2; each goes through the "%.1f" text round trip:  q = v * 10, k = rint(q); if q is
//      exactly a half-integer and the exact residual fma(v, 10, -q) is not zero, k is the neighbour on the residual's side; the
//      value is float32(k / 10.0).  NaN and +-inf pass through.  Raw mode (mode 1): the float32 points as they are, in their order.
//   3. spline (spline_interp_times(lane, 50), operation for operation).  n >= 3: d[i] = p[i+1] - p[i], h[i] = sqrt(dx*dx + dy*dy),
//      A[i] = h[i], B[i] = 2 * (h[i] + h[i+1]), C[i] = h[i+1], D[i] = 6 * (d[i+1] / h[i+1] - d[i] / h[i]);  C[0] /= B[0],
//      D[0] /= B[0];  i = 1 .. n-3: tmp = B[i] - A[i] * C[i-1], C[i] /= tmp, D[i] = (D[i] - A[i] * D[i-1]) / tmp;  M[n-2] = D[n-3],
//      i = n-4 .. 0: M[i+1] = D[i] - C[i] * M[i+2];  M[0] = M[n-1] = 0.  Interval i, k = 0 .. 49: t = (h[i] / 50) * k,
//      b = d[i] / h[i] - ((2 * h[i]) * M[i] + h[i] * M[i+1]) / 6, c = M[i] / 2, dd = (M[i+1] - M[i]) / (6 * h[i]),
//      point = float32(p[i] + b * t + c * (t * t) + dd * ((t * t) * t)); the last input point is appended.  n == 2: the two points.
//      n < 2: no segments.  A repeated point gives h = 0, NaN coefficients and, by rule 4, end points 0.
//   4. end points (lane_segments).  float32 -> double, NaN -> 0, rint (ties to even), clamp to +-8192.  Consecutive points are the
//      rows (x0, y0, x1, y1, lane); a lane's rows start at lane * C, its unused rows carry lane -1 (phnet_lane_raster skips them).
// One workgroup per lane: threads 0 and 1 solve the x and the y system in LDS, all 256 evaluate the intervals.
//
// Count rules, per image (count_im_pair on make_match, exactly as written there):
//   the present annotations / predictions (lane_pts >= 0) are compacted in order: n_anno rows, n_detect columns;
//   sim[r][c] = 0 where either lane has fewer than 2 points, else the iou entry (NaN stays NaN);
//   n_anno == 0 and n_detect == 0: iou_im = 1;  n_anno == 0: fp = n_detect;  n_detect == 0: fn = n_anno (iou_im = 0 in both);
//   else Kuhn-Munkres on sim (transposed when n_anno > n_detect): left weights start at -1e5 and take `w < m ? m : w` over the row,
//   right weights at 0; an edge is tight iff |lw + rw - m| < 1e-2; the depth-first search visits columns in ascending order
//   (_augment); after a failed search dmin = 1e10, then `d < dmin ? d : dmin` over (visited row, unvisited column); dmin == 1e10
//   ends the matching, otherwise visited rows lose dmin and visited columns gain it.  A matched annotation adds its sim to the sum;
//   it is a true positive iff sim > threshold, else its match is withdrawn.  iou_im = sum / n_detect.
//   The relabelling passes of one image are capped at PHNET_LANE_EVAL_RELABEL_CAP; an image that needs more counts as unmatched
//   (tp = 0, iou_im = 0) and increments `overflow`.
// One workgroup of 64 threads walks the images (thread t takes images t, t + 64, ...; the state of a matching lives in LDS); after
// a barrier thread 0 adds the images to the totals in ascending order - the host's summation order, whatever the scheduling.
#include "common.h"
#include "../../include/phnet_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxSide = PHNET_LANE_EVAL_MAX_LANES;        // G, L
constexpr int kMaxPts = PHNET_LANE_EVAL_MAX_POINTS;        // S, P
constexpr int kTimes = 50;
constexpr double kCoord = 8192.0;
constexpr double kDblMax = 1.79769313486231570e308;

// the value read_lane_file returns for the text "%.1f" % v
__device__ __forceinline__ double text_round_trip(double v)
{
    if (!(fabs(v) <= kDblMax)) return v;                             // NaN, +-inf
    const double q = v * 10.0;
    double k = rint(q);
    const double fl = floor(q);
    if (q - fl == 0.5) {                                             // exact: q below 2^52 here, a larger q is an integer
        const double r = fma(v, 10.0, -q);                           // v * 10 - q without rounding
        if (r > 0.0) k = fl + 1.0;
        else if (r < 0.0) k = fl;
    }
    return (double)(float)(k / 10.0);
}

__device__ __forceinline__ int end_point(float v)
{
    double d = (double)v;
    if (d != d) d = 0.0;
    d = rint(d);
    d = d < -kCoord ? -kCoord : (d > kCoord ? kCoord : d);
    return (int)d;
}

__global__ __launch_bounds__(256) void lane_eval_segments_kernel(const float* __restrict__ points, const int* __restrict__ count,
                                                                 const int* __restrict__ lanes_num, const float* __restrict__ gt_points,
                                                                 const int* __restrict__ gt_count, const int* __restrict__ gt_num,
                                                                 int G, int L, int S, int P, int C, int mode, double size_h,
                                                                 double size_w, double crop_top, int* __restrict__ segs,
                                                                 int* __restrict__ lane_pts)
{
    __shared__ double s_p[2][kMaxPts], s_h[kMaxPts], s_c[2][kMaxPts], s_d[2][kMaxPts], s_m[2][kMaxPts];
    const int tid = threadIdx.x;
    const long lane = blockIdx.x;
    const long f = lane / (G + L);
    const int j = (int)(lane % (G + L));

    // ---- rule 1: presence and point count (every count clamped before it indexes anything) ----
    int n;
    bool present;
    const float* src;
    bool wire = false;
    if (j < G) {
        const int gn = min(max(gt_num[f], 0), G);
        n = min(max(gt_count[f * G + j], 0), P);
        present = j < gn;
        src = gt_points + (f * G + j) * (long)P * 2;
    } else {
        const int k = j - G;
        const int ln = min(max(lanes_num[f], 0), L);
        n = min(max(count[f * L + k], 0), S);
        wire = mode == 0;
        present = k < ln && (!wire || n > 2);
        src = points + (f * L + k) * (long)S * 2;
    }
    if (tid == 0) lane_pts[lane] = present ? n : -1;
    int* rows = segs + lane * (long)C * 5;
    const int n_seg = !present || n < 2 ? 0 : (n == 2 ? 1 : (n - 1) * kTimes);       // <= C
    if (n_seg == 0) {
        for (int i = tid; i < C; i += blockDim.x) {
            int* r = rows + (long)i * 5;
            r[0] = 0; r[1] = 0; r[2] = 0; r[3] = 0; r[4] = -1;
        }
        return;
    }

    // ---- rule 2: the lane's points in evaluator coordinates ----
    for (int i = tid; i < n; i += blockDim.x) {
        if (wire) {
            const float* q = src + (long)(n - 1 - i) * 2;
            s_p[0][i] = text_round_trip(((double)q[0] * size_w) / 2.0);
            s_p[1][i] = text_round_trip(((double)q[1] * size_h + crop_top) / 2.0);
        } else {
            s_p[0][i] = (double)src[(long)i * 2];
            s_p[1][i] = (double)src[(long)i * 2 + 1];
        }
    }
    __syncthreads();

    // ---- rule 3: chord lengths, right-hand sides, the tridiagonal solve as written ----
    if (n >= 3) {
        for (int i = tid; i < n - 1; i += blockDim.x) {
            const double dx = s_p[0][i + 1] - s_p[0][i], dy = s_p[1][i + 1] - s_p[1][i];
            s_h[i] = sqrt(dx * dx + dy * dy);
        }
        __syncthreads();
        for (int i = tid; i < n - 2; i += blockDim.x) {
            const double h0 = s_h[i], h1 = s_h[i + 1];
#pragma unroll
            for (int a = 0; a < 2; ++a)
                s_d[a][i] = 6.0 * ((s_p[a][i + 2] - s_p[a][i + 1]) / h1 - (s_p[a][i + 1] - s_p[a][i]) / h0);
        }
        __syncthreads();
        if (tid < 2) {                                               // thread 0: x, thread 1: y, each with its own copy of C
            double* c = s_c[tid];
            double* d = s_d[tid];
            double* m = s_m[tid];
            const double b0 = 2.0 * (s_h[0] + s_h[1]);
            c[0] = s_h[1] / b0;
            d[0] = d[0] / b0;
            for (int i = 1; i < n - 2; ++i) {
                const double a = s_h[i];
                const double tmp = 2.0 * (s_h[i] + s_h[i + 1]) - a * c[i - 1];
                c[i] = s_h[i + 1] / tmp;
                d[i] = (d[i] - a * d[i - 1]) / tmp;
            }
            m[n - 2] = d[n - 3];
            for (int i = n - 4; i >= 0; --i) m[i + 1] = d[i] - c[i] * m[i + 2];
            m[0] = 0.0;
            m[n - 1] = 0.0;
        }
        __syncthreads();
    }

    // ---- rules 3 and 4: polyline point q of the lane, rounded to its cv::line end point ----
    auto poly = [&](int q, int a) -> int {
        if (n == 2) return end_point((float)s_p[a][q]);
        const int iv = q / kTimes, k = q - iv * kTimes;
        if (iv >= n - 1) return end_point((float)s_p[a][n - 1]);      // the appended last point
        const double h = s_h[iv], m0 = s_m[a][iv], m1 = s_m[a][iv + 1], p0 = s_p[a][iv];
        const double t = (h / (double)kTimes) * (double)k;
        const double b = (s_p[a][iv + 1] - p0) / h - ((2.0 * h) * m0 + h * m1) / 6.0;
        const double c = m0 / 2.0;
        const double dd = (m1 - m0) / (6.0 * h);
        const double t2 = t * t;
        return end_point((float)(p0 + b * t + c * t2 + dd * (t2 * t)));
    };
    for (int i = tid; i < C; i += blockDim.x) {
        int* r = rows + (long)i * 5;
        if (i < n_seg) {
            r[0] = poly(i, 0); r[1] = poly(i, 1); r[2] = poly(i + 1, 0); r[3] = poly(i + 1, 1); r[4] = (int)lane;
        } else {
            r[0] = 0; r[1] = 0; r[2] = 0; r[3] = 0; r[4] = -1;
        }
    }
}

__global__ __launch_bounds__(64) void lane_eval_count_kernel(const double* __restrict__ iou, const int* __restrict__ lane_pts, int F,
                                                             int G, int L, double threshold, const int* __restrict__ video, int V,
                                                             int* __restrict__ tp, int* __restrict__ fp, int* __restrict__ fn,
                                                             double* __restrict__ iou_im, int* __restrict__ anno_match,
                                                             long long* __restrict__ totals, double* __restrict__ iou_tot,
                                                             int* __restrict__ overflow)
{
    // per-thread state of one matching, [index][thread]: a thread's words sit in its own bank column
    __shared__ double s_lw[kMaxSide][64], s_rw[kMaxSide][64];
    __shared__ signed char s_row[kMaxSide][64], s_col[kMaxSide][64], s_lm[kMaxSide][64], s_rm[kMaxSide][64];
    __shared__ signed char s_sx[kMaxSide + 1][64], s_sv[kMaxSide + 1][64], s_sp[kMaxSide + 1][64];
    __shared__ int s_over;
    const int t = threadIdx.x;
    if (t == 0) s_over = 0;
    __syncthreads();

    for (int f = t; f < F; f += 64) {
        const int* lp = lane_pts + (long)f * (G + L);
        const double* m = iou + (long)f * G * L;
        int* am = anno_match + (long)f * G;
        int na = 0, nd = 0;
        for (int g = 0; g < G; ++g) {
            am[g] = -1;
            if (lp[g] >= 0) s_row[na++][t] = (signed char)g;
        }
        for (int k = 0; k < L; ++k)
            if (lp[G + k] >= 0) s_col[nd++][t] = (signed char)k;
        auto sim = [&](int r, int c) -> double {
            const int g = s_row[r][t], k = s_col[c][t];
            return (lp[g] < 2 || lp[G + k] < 2) ? 0.0 : m[g * L + k];
        };
        int n_tp = 0;
        double im = 0.0;
        if (na == 0 && nd == 0) {
            im = 1.0;
        } else if (na != 0 && nd != 0) {
            const bool swap = na > nd;
            const int LL = swap ? nd : na, RR = swap ? na : nd;
            auto mat = [&](int i, int j2) -> double { return swap ? sim(j2, i) : sim(i, j2); };
            for (int i = 0; i < LL; ++i) {
                double w = -1e5;
                for (int j2 = 0; j2 < RR; ++j2) {
                    const double v = mat(i, j2);
                    if (w < v) w = v;
                }
                s_lw[i][t] = w;
                s_lm[i][t] = -1;
            }
            for (int j2 = 0; j2 < RR; ++j2) { s_rw[j2][t] = 0.0; s_rm[j2][t] = -1; }
            int relabels = 0;
            bool done = false, over = false;
            for (int u = 0; u < LL && !done && !over; ++u) {
                for (;;) {
                    unsigned lu = 1u << u, ru = 0u;
                    // _augment(u): the recursion of matchDfs as a stack of (row, next column, column taken)
                    bool ok = false;
                    int sp = 0;
                    s_sx[0][t] = (signed char)u; s_sv[0][t] = 0; s_sp[0][t] = -1;
                    while (sp >= 0 && !ok) {
                        const int x = s_sx[sp][t];
                        int v = s_sv[sp][t];
                        bool advanced = false;
                        for (; v < RR; ++v) {
                            if (((ru >> v) & 1u) || !(fabs(s_lw[x][t] + s_rw[v][t] - mat(x, v)) < 1e-2)) continue;
                            ru |= 1u << v;
                            const int child = s_rm[v][t];
                            if (child == -1) {
                                s_rm[v][t] = (signed char)x; s_lm[x][t] = (signed char)v;
                                for (--sp; sp >= 0; --sp) {
                                    const int px = s_sx[sp][t], pv = s_sp[sp][t];
                                    s_rm[pv][t] = (signed char)px; s_lm[px][t] = (signed char)pv;
                                }
                                ok = true;
                                break;
                            }
                            s_sv[sp][t] = (signed char)(v + 1); s_sp[sp][t] = (signed char)v;
                            lu |= 1u << child;
                            ++sp;                                    // <= the columns marked so far <= kMaxSide
                            s_sx[sp][t] = (signed char)child; s_sv[sp][t] = 0; s_sp[sp][t] = -1;
                            advanced = true;
                            break;
                        }
                        if (!ok && !advanced) --sp;
                    }
                    if (ok) break;
                    double dmin = 1e10;
                    for (int i = 0; i < LL; ++i) {
                        if (!((lu >> i) & 1u)) continue;
                        for (int j2 = 0; j2 < RR; ++j2) {
                            if ((ru >> j2) & 1u) continue;
                            const double d = s_lw[i][t] + s_rw[j2][t] - mat(i, j2);
                            dmin = d < dmin ? d : dmin;
                        }
                    }
                    if (dmin == 1e10) { done = true; break; }
                    if (++relabels > PHNET_LANE_EVAL_RELABEL_CAP) { over = true; break; }
                    for (int i = 0; i < LL; ++i) if ((lu >> i) & 1u) s_lw[i][t] -= dmin;
                    for (int j2 = 0; j2 < RR; ++j2) if ((ru >> j2) & 1u) s_rw[j2][t] += dmin;
                }
            }
            if (over) {
                atomicAdd(&s_over, 1);
            } else {
                double sum = 0.0;
                for (int i = 0; i < na; ++i) {
                    const int c = swap ? s_rm[i][t] : s_lm[i][t];
                    if (c < 0) continue;
                    const double s = sim(i, c);
                    sum += s;
                    if (s > threshold) { ++n_tp; am[s_row[i][t]] = s_col[c][t]; }
                }
                im = sum / (double)nd;
            }
        }
        tp[f] = n_tp; fp[f] = nd - n_tp; fn[f] = na - n_tp; iou_im[f] = im;
    }
    __threadfence();
    __syncthreads();
    if (t == 0) {                                                    // ascending f: the host's order of `iou += d`
        for (int f = 0; f < F; ++f) {
            const int v = video ? video[f] : 0;
            if ((unsigned)v >= (unsigned)V) continue;                // an image of no video row is in no total
            totals[v * 4L + 0] += tp[f]; totals[v * 4L + 1] += fp[f]; totals[v * 4L + 2] += fn[f]; totals[v * 4L + 3] += 1;
            iou_tot[v] += iou_im[f];
        }
        overflow[0] += s_over;
    }
}

bool finite_arg(double v) { return v >= -kDblMax && v <= kDblMax; }

}  // namespace

PHNET_API int phnet_lane_eval_segments(const float* points, const int32_t* count, const int32_t* lanes_num, const float* gt_points,
                                       const int32_t* gt_count, const int32_t* gt_num, int64_t F, int32_t G, int32_t L, int32_t S,
                                       int32_t P, int32_t mode, double size_h, double size_w, double crop_top, int32_t* segs,
                                       int32_t* lane_pts, void* stream)
{
    if (!points || !count || !lanes_num || !gt_points || !gt_count || !gt_num || !segs || !lane_pts) return PHNET_ERR_ARG;
    if (F < 1 || G < 1 || G > kMaxSide || L < 1 || L > kMaxSide || S < 2 || S > kMaxPts || P < 2 || P > kMaxPts) return PHNET_ERR_ARG;
    if ((mode != 0 && mode != 1) || !finite_arg(size_h) || !finite_arg(size_w) || !finite_arg(crop_top)) return PHNET_ERR_ARG;
    const int64_t C = (int64_t)((S > P ? S : P) - 1) * kTimes;
    if (F > 0x7fffffffll / ((G + L) * C)) return PHNET_ERR_ARG;                 // F * (G + L) * C < 2^31: row and lane numbers are int32
    hipLaunchKernelGGL(lane_eval_segments_kernel, dim3((unsigned)(F * (G + L))), dim3(256), 0, (hipStream_t)stream, points, count,
                       lanes_num, gt_points, gt_count, gt_num, (int)G, (int)L, (int)S, (int)P, (int)C, (int)mode, size_h, size_w,
                       crop_top, segs, lane_pts);
    return phnet_launch_status();
}

PHNET_API int phnet_lane_eval_count(const double* iou, const int32_t* lane_pts, int64_t F, int32_t G, int32_t L, double threshold,
                                    const int32_t* video, int32_t V, int32_t* tp, int32_t* fp, int32_t* fn, double* iou_im,
                                    int32_t* anno_match, int64_t* totals, double* iou_tot, int32_t* overflow, void* stream)
{
    if (!iou || !lane_pts || !tp || !fp || !fn || !iou_im || !anno_match || !totals || !iou_tot || !overflow) return PHNET_ERR_ARG;
    if (F < 1 || F > 0x7fffffffll / (2 * kMaxSide * kMaxSide) || G < 1 || G > kMaxSide || L < 1 || L > kMaxSide || V < 1)
        return PHNET_ERR_ARG;
    hipLaunchKernelGGL(lane_eval_count_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, iou, lane_pts, (int)F, (int)G, (int)L,
                       threshold, video, (int)V, tp, fp, fn, iou_im, anno_match, (long long*)totals, iou_tot, overflow);
    return phnet_launch_status();
}
