// Lane-IoU kernels of the CULane-style evaluator (reference: evaluation/culane/src/lane_compare.cpp:11-57 - draw both lanes
// as thick poly-lines, count pixels, IoU = |A & B| / |A | B|).  A lane is a bit mask [height][ceil(width / 32)] words in HBM:
// `lane_raster_kernel` ORs one thick segment per workgroup into its lane's mask, `lane_mask_stats_kernel` counts the bits of
// every lane and of every requested pair's intersection, `lane_iou_groups_kernel` turns the masks into whole IoU matrices (one
// workgroup per entry; the temporal evaluator, evaluation/evalTemporalOLV2.py:26-35).  Pixel rule (oracle/culane_cpu.py raster_lane, exact integers): the
// pixel centre lies within lane_width / 2 of the segment between the integer end points - the ideal shape of cv::line's
// quadrilateral + end circles (parity against OpenCV's scan conversion unpinned: OpenCV is not in the reference tree).
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void lane_raster_kernel(const int* __restrict__ segs, long n_segs, unsigned* __restrict__ masks,
                                                          int n_lanes, int height, int width, int lane_width)
{
    const long s = blockIdx.x;
    if (s >= n_segs) return;
    const int x0 = segs[s * 5 + 0], y0 = segs[s * 5 + 1], x1 = segs[s * 5 + 2], y1 = segs[s * 5 + 3], lane = segs[s * 5 + 4];
    if ((unsigned)lane >= (unsigned)n_lanes) return;
    const int r = (lane_width + 1) / 2;
    const int xa = max(0, min(x0, x1) - r), xb = min(width - 1, max(x0, x1) + r);
    const int ya = max(0, min(y0, y1) - r), yb = min(height - 1, max(y0, y1) + r);
    if (xa > xb || ya > yb) return;
    const int wpr = (width + 31) >> 5;                               // words per mask row
    const int wa = xa >> 5, wb = xb >> 5, nw = wb - wa + 1;
    const long dx = x1 - x0, dy = y1 - y0, L2 = dx * dx + dy * dy, w2 = (long)lane_width * lane_width;
    unsigned* m = masks + (size_t)lane * height * wpr;
    for (int item = threadIdx.x; item < (yb - ya + 1) * nw; item += blockDim.x) {
        const int y = ya + item / nw, w = wa + item % nw;
        const long qy = y - y0, ey = y - y1;
        unsigned bits = 0;
        for (int b = 0; b < 32; ++b) {
            const int x = w * 32 + b;
            if (x < xa || x > xb) continue;
            const long qx = x - x0, ex = x - x1;
            const long dot = qx * dx + qy * dy;
            bool in;
            if (dot <= 0) in = 4 * (qx * qx + qy * qy) <= w2;
            else if (dot >= L2) in = 4 * (ex * ex + ey * ey) <= w2;
            else { const long c = qx * dy - qy * dx; in = 4 * c * c <= w2 * L2; }
            bits |= in ? 1u << b : 0u;
        }
        if (bits) atomicOr(m + (size_t)y * wpr + w, bits);
    }
}

// blockIdx.y < n_lanes: area of that lane; else pair blockIdx.y - n_lanes: bits of the intersection
__global__ __launch_bounds__(256) void lane_mask_stats_kernel(const unsigned* __restrict__ masks, int n_lanes, long words,
                                                              const int* __restrict__ pairs, int n_pairs,
                                                              unsigned long long* __restrict__ area, unsigned long long* __restrict__ inter)
{
    const int job = blockIdx.y;
    const unsigned *a, *b;
    unsigned long long* dst;
    if (job < n_lanes) { a = b = masks + (size_t)job * words; dst = area + job; }
    else {
        const int p = job - n_lanes, i = pairs[2 * p], j = pairs[2 * p + 1];
        if ((unsigned)i >= (unsigned)n_lanes || (unsigned)j >= (unsigned)n_lanes) return;
        a = masks + (size_t)i * words; b = masks + (size_t)j * words; dst = inter + p;
    }
    unsigned cnt = 0;
    for (long w = (long)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (long)gridDim.x * blockDim.x) cnt += __popc(a[w] & b[w]);
    float f = (float)cnt;                                            // < 2^24 per wave: exact
    f = wave_sum(f);
    __shared__ unsigned part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = (unsigned)f;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = part[0] + part[1] + part[2] + part[3];
        if (t) atomicAdd(dst, (unsigned long long)t);
    }
}

// One workgroup per job.  job < n_entries: entry `job` of the IoU matrices - the group is the last one whose out_first <= job
// (binary search; empty groups share their out_first with the next group and are never chosen), (r, c) the position in it.
// job >= n_entries (only launched with `area`): the area of lane job - n_entries.  Both masks are read once, I = |a & b|,
// A = |a| and B = |b| in the same pass (128-bit loads at 4-byte alignment - a lane's mask starts at any word - plus a
// scalar tail of words % 4).  Per-wave counts stay below 64 * 2048 * 32 = 2^22 (words <= 4096 * 128), exact in the float
// wave_sum.  Every job writes its own element once: no atomics, no zeroed output.
typedef unsigned mask_quad __attribute__((ext_vector_type(4), aligned(4)));

__global__ __launch_bounds__(256) void lane_iou_groups_kernel(const unsigned* __restrict__ masks, int n_lanes, long words,
                                                              const int* __restrict__ groups, int n_groups, long n_entries,
                                                              long scale, double eps, double* __restrict__ iou,
                                                              long long* __restrict__ area)
{
    const long job = blockIdx.x;
    int i, j;
    if (job < n_entries) {
        int lo = 0, hi = n_groups - 1;                               // out_first[0] = 0 <= job
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((long)groups[mid * 5 + 4] <= job) lo = mid; else hi = mid - 1;
        }
        const int* g = groups + (size_t)lo * 5;
        const long k = job - g[4], nc = g[3];
        if (k < 0 || nc < 1 || k >= (long)g[1] * nc) return;          // a table that does not cover this entry
        i = g[0] + (int)(k / nc); j = g[2] + (int)(k % nc);
    } else {
        i = j = (int)(job - n_entries);
    }
    if ((unsigned)i >= (unsigned)n_lanes || (unsigned)j >= (unsigned)n_lanes) return;
    const unsigned* a = masks + (size_t)i * words;
    const unsigned* b = masks + (size_t)j * words;
    const mask_quad* a4 = (const mask_quad*)a;
    const mask_quad* b4 = (const mask_quad*)b;
    const long quads = words >> 2;
    unsigned ci = 0, ca = 0, cb = 0;
    for (long q = threadIdx.x; q < quads; q += blockDim.x) {
        const mask_quad x = a4[q], y = b4[q];
        ci += __popc(x.x & y.x) + __popc(x.y & y.y) + __popc(x.z & y.z) + __popc(x.w & y.w);
        ca += __popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w);
        cb += __popc(y.x) + __popc(y.y) + __popc(y.z) + __popc(y.w);
    }
    for (long w = (quads << 2) + threadIdx.x; w < words; w += blockDim.x) {
        const unsigned x = a[w], y = b[w];
        ci += __popc(x & y); ca += __popc(x); cb += __popc(y);
    }
    const float fi = wave_sum((float)ci), fa = wave_sum((float)ca), fb = wave_sum((float)cb);
    __shared__ unsigned part[3][4];
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = (unsigned)fi; part[1][threadIdx.x >> 6] = (unsigned)fa; part[2][threadIdx.x >> 6] = (unsigned)fb;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long I = (long)part[0][0] + part[0][1] + part[0][2] + part[0][3];
        const long A = (long)part[1][0] + part[1][1] + part[1][2] + part[1][3];
        const long B = (long)part[2][0] + part[2][1] + part[2][2] + part[2][3];
        if (job < n_entries) iou[job] = (double)(scale * I) / ((double)(scale * (A + B - I)) + eps);   // integers, then one add, one divide
        else area[i] = A;
    }
}

}  // namespace

// segs [n_segs][5] int32 (x0, y0, x1, y1, lane); masks [n_lanes][height][ceil(width / 32)] uint32, zeroed by the caller (bits are ORed in)
PHNET_API int phnet_lane_raster(const int32_t* segs, int64_t n_segs, uint32_t* masks, int32_t n_lanes, int32_t height, int32_t width,
                                int32_t lane_width, void* stream)
{
    if (n_segs < 0 || n_lanes < 0 || height < 1 || width < 1 || height > 4096 || width > 4096 || lane_width < 1 || lane_width > 256)
        return PHNET_ERR_ARG;                       // with end points inside +-2^13 the 64-bit distance tests cannot overflow
    if (n_segs == 0 || n_lanes == 0) return PHNET_OK;
    if (!segs || !masks || n_segs > 0x7fffffffL) return PHNET_ERR_ARG;
    hipLaunchKernelGGL(lane_raster_kernel, dim3((unsigned)n_segs), dim3(256), 0, (hipStream_t)stream,
                       segs, (long)n_segs, masks, n_lanes, height, width, lane_width);
    return phnet_launch_status();
}

// area [n_lanes] and inter [n_pairs] int64, zeroed by the caller: set bits of every lane mask / of masks[pairs[p][0]] & masks[pairs[p][1]]
PHNET_API int phnet_lane_mask_stats(const uint32_t* masks, int32_t n_lanes, int32_t height, int32_t width, const int32_t* pairs,
                                    int32_t n_pairs, int64_t* area, int64_t* inter, void* stream)
{
    if (n_lanes < 0 || n_pairs < 0 || height < 1 || width < 1) return PHNET_ERR_ARG;
    if (n_lanes + n_pairs == 0) return PHNET_OK;
    if (!masks || !area || (n_pairs && (!pairs || !inter)) || n_lanes + n_pairs > 65535) return PHNET_ERR_ARG;
    const long words = (long)height * ((width + 31) >> 5);
    const unsigned bx = (unsigned)min((long)64, ceil_div64(words, 256 * 8));
    hipLaunchKernelGGL(lane_mask_stats_kernel, dim3(bx, (unsigned)(n_lanes + n_pairs)), dim3(256), 0, (hipStream_t)stream,
                       masks, n_lanes, words, pairs, n_pairs, (unsigned long long*)area, (unsigned long long*)inter);
    return phnet_launch_status();
}

// IoU matrices straight from the masks (include/phnet_hip.h): one workgroup per matrix entry (+ one per lane when `area` is given)
PHNET_API int phnet_lane_iou_groups(const uint32_t* masks, int32_t n_lanes, int32_t height, int32_t width, const int32_t* groups,
                                    int32_t n_groups, int64_t n_entries, int32_t scale, double eps, double* iou, int64_t* area,
                                    void* stream)
{
    if (n_lanes < 0 || n_groups < 0 || n_entries < 0 || height < 1 || width < 1 || height > 4096 || width > 4096 || scale < 1 ||
        !(eps >= 0.0) || eps > 1.79769313486231570e308)                 // !(>=) also refuses a NaN
        return PHNET_ERR_ARG;
    if (n_groups == 0) n_entries = 0;
    const int64_t jobs = n_entries + (area ? n_lanes : 0);
    if (jobs == 0) return PHNET_OK;
    if (!masks || (n_entries && (!groups || !iou)) || jobs > 0x7fffffffL) return PHNET_ERR_ARG;
    const long words = (long)height * ((width + 31) >> 5);
    hipLaunchKernelGGL(lane_iou_groups_kernel, dim3((unsigned)jobs), dim3(256), 0, (hipStream_t)stream,
                       masks, n_lanes, words, groups, n_groups, (long)n_entries, (long)scale, eps, iou, (long long*)area);
    return phnet_launch_status();
}
