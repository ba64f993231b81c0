// Lanes back onto a picture, on the device: the polylines of phnet_lane_points -> a label map (one byte per pixel, one value per
// lane or per track) and / or an overlay on the camera frame, for F frames in one launch (DESIGN.md "Lane overlay"; the numbered
// rules are in include/phnet_hip.h).  Replaces the host loops of the reference's test script (testOL.py:165-227: predlanesV2 and
// generate_seg_from_line map every point with int(), draw with cv2.line(thickness = 12) lane by lane; libs/utils/utility.py:66-68
// blends 50/50 with the input) for callers that want the picture where the rest of the step already is.
//
// Pixel rule: the project's own (oracle/culane_cpu.py raster_lane, csrc/lane_iou.hip) - a pixel belongs to a segment when its
// centre lies within lane_width / 2 of the segment between the INTEGER end points, 4 d^2 <= lane_width^2 in exact integers; the
// ideal shape of cv::line's quadrilateral + end circles.  PARITY UNPINNED against cv2.line's scan conversion (OpenCV is not in the
// reference tree), the caveat lane_iou.hip carries for the same rule.
//
// Shape: a workgroup of 256 threads owns a tile of 128 x 8 output pixels of one frame, a thread four horizontally adjacent ones.
//   1. lane boxes, one wavefront per lane: the box of the lane's surviving points, grown by (lane_width + 1) / 2, against the tile.
//      A lane far from the tile costs this one test and nothing after it.
//   2. the lanes that passed, from the highest packed index k down, one after the other with the whole workgroup (thread t owns
//      point t): survivors pair up with their predecessors (ballots), the segments whose grown box meets the tile are appended to
//      a list in LDS, in order.  When the list could not take another lane (1024 entries; a lane has at most 255 segments) the
//      pixels are resolved against it and it is emptied - pixels that found their lane stay found, so the order rule holds across
//      the flush.
//   3. resolve: every thread walks the list from its start (highest k first) and stops at the first hit of each of its pixels.
//   4. every thread stores its pixels EXACTLY ONCE with plain vector stores: one dword of labels and three of RGB where bases and
//      row lengths are multiples of four (WIDE), bytes otherwise.  No atomics, no clearing pass: a replayed graph cannot show a
//      lane of the previous frame and the result does not depend on scheduling.
//
// The coordinate bound: a point whose pixel coordinate lies outside [-8192, 8192] is skipped (rule 1).  With end points inside
// that bound and pixels inside [0, 4096): |q| = |pixel - end point| <= 4095 + 8192 < 2^14 and |d| = |end - end| <= 2^14 per axis, so
// dot = qx dx + qy dy, L2 = dx^2 + dy^2, d0 = qx^2 + qy^2 and cross = qx dy - qy dx are all below 2 * 2^28 = 2^29 in magnitude:
// 4 d0 <= 2^31, 4 cross^2 <= 2^60 and lane_width^2 L2 <= 2^16 * 2^29 = 2^45 - every product of raster_lane's int64 test stays
// below 2^63.  Here the first-order terms are 32-bit (24-bit multiplies of operands below 2^15: exact, full rate) and only
// cross^2 and lane_width^2 L2 are 64-bit; the integers are the same.
#include "common.h"
#include "csc.h"

namespace {

constexpr int NT = 256;                       // threads of a workgroup = the most points a lane has (S <= 256): thread t owns point t
constexpr int TW = 128, TH = 8, PX = 4;       // tile of a workgroup; pixels of a thread
constexpr int kMaxLanes = 64, kMaxOffsets = 256;   // L, S: the limits of phnet_lane_points
constexpr int kCap = 1024;                    // segments the LDS list holds between two flushes
constexpr int kCoordBound = 8192;             // rule 1

struct DrawArgs {
    const float2* points; const int* count; const int* lanes_num; const int* slot; const int* track_id;
    int L, S;
    double sx, sy, oy;
    int out_h, out_w, lane_width;
    const uint8_t* src; long frame_stride; unsigned pitch, chroma_offset; Csc k;
    const uint8_t* palette; int alpha;
    uint8_t* label; uint8_t* overlay;
    unsigned tiles_x, tiles_per_frame;
};

// rule 1.  Two roundings for y, as Python's y * sy + oy: nothing is contracted.
__device__ __forceinline__ bool map_point(float2 p, double sx, double sy, double oy, int& px, int& py)
{
    if (!(p.x > 0.f) || !(p.y > 0.f)) return false;                               // x <= 0, y <= 0, NaN
    const double fx = __dmul_rn((double)p.x, sx);
    const double fy = __dadd_rn(__dmul_rn((double)p.y, sy), oy);
    const double lim = (double)(kCoordBound + 1);                                  // |trunc(v)| <= 8192 iff |v| < 8193; false for NaN, +-inf
    if (!(fx > -lim && fx < lim && fy > -lim && fy < lim)) return false;
    px = (int)fx; py = (int)fy;                                                    // truncates toward zero
    return true;
}

template <int CTRL>
__device__ __forceinline__ int dpp_move_i(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false); }

// the DPP sequence of wave_sum (common.h) on an idempotent operation: lane 63 ends with the result of all 64 lanes
__device__ __forceinline__ int wave_min_i(int v) {
    v = min(v, dpp_move_i<0xb1>(v)); v = min(v, dpp_move_i<0x4e>(v)); v = min(v, dpp_move_i<0x124>(v));
    v = min(v, dpp_move_i<0x128>(v)); v = min(v, dpp_move_i<0x142>(v)); v = min(v, dpp_move_i<0x143>(v));
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ int wave_max_i(int v) {
    v = max(v, dpp_move_i<0xb1>(v)); v = max(v, dpp_move_i<0x4e>(v)); v = max(v, dpp_move_i<0x124>(v));
    v = max(v, dpp_move_i<0x128>(v)); v = max(v, dpp_move_i<0x142>(v)); v = max(v, dpp_move_i<0x143>(v));
    return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ int byte_of(unsigned w, int i) { return (int)((w >> (8 * i)) & 0xffu); }

// FMT: the source under the overlay - 0 none (black), 1 packed RGB rows of `pitch` bytes, 2 NV12, 3 YUYV (the surfaces of
// phnet_preprocess_yuv).  WIDE: every base, stride and row length is a multiple of four, so four pixels are whole dwords.
template <int FMT, bool WIDE>
__global__ __launch_bounds__(NT) void lane_draw_kernel(const DrawArgs a)
{
    __shared__ int4 s_list[kCap];                    // (x0 | y0 << 16, x1 | y1 << 16, value, -), highest lane first
    __shared__ int s_pts[kMaxOffsets];               // pixel of point t of the lane in hand, x | y << 16
    __shared__ unsigned long long s_mask[NT / 64];   // its survivors, per wavefront
    __shared__ int s_hcnt[NT / 64];                  // segments of it that meet the tile, per wavefront
    __shared__ int s_hit[kMaxLanes];                 // phase 1: lane k's grown box meets the tile
    __shared__ uint8_t s_pal[768];

    const unsigned f = blockIdx.x / a.tiles_per_frame, tile = blockIdx.x - f * a.tiles_per_frame;
    const int tile_y = (int)(tile / a.tiles_x), tile_x = (int)(tile - (unsigned)tile_y * a.tiles_x);
    const int X0 = tile_x * TW, Y0 = tile_y * TH;
    const int X1 = min(X0 + TW, a.out_w) - 1, Y1 = min(Y0 + TH, a.out_h) - 1;     // the tile's last column and row inside the image
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int L = a.L, S = a.S;
    const int r = (a.lane_width + 1) / 2, w2 = a.lane_width * a.lane_width;
    const float2* pts = a.points + (size_t)f * L * S;
    const int* cnts = a.count + (size_t)f * L;

    if (a.overlay)
        for (int i = t; i < 768; i += NT) s_pal[i] = a.palette[i];
    const int n_raw = a.lanes_num[f];
    const int n = n_raw < 0 ? 0 : (n_raw > L ? L : n_raw);

    // ---- phase 1: lane boxes against the tile, one wavefront per lane ----
    for (int k = wave; k < n; k += NT / 64) {
        const int c_raw = cnts[k];
        const int c = c_raw < 0 ? 0 : (c_raw > S ? S : c_raw);
        int xmin = INT32_MAX, xmax = INT32_MIN, ymin = INT32_MAX, ymax = INT32_MIN, alive = 0;
        for (int base = 0; base < c; base += 64) {                                 // wave-uniform trip count
            const int i = base + lane;
            int px = 0, py = 0;
            const bool ok = i < c && map_point(pts[(size_t)k * S + i], a.sx, a.sy, a.oy, px, py);
            if (ok) { xmin = min(xmin, px); xmax = max(xmax, px); ymin = min(ymin, py); ymax = max(ymax, py); }
            alive += __popcll(__ballot(ok));
        }
        xmin = wave_min_i(xmin); xmax = wave_max_i(xmax); ymin = wave_min_i(ymin); ymax = wave_max_i(ymax);
        if (lane == 0)
            s_hit[k] = alive >= 2 && xmin - r <= X1 && xmax + r >= X0 && ymin - r <= Y1 && ymax + r >= Y0;
    }
    __syncthreads();

    // this thread's pixels: row y, columns x0 .. x0 + 3; v[j] = 0 until a lane covers pixel j
    const int y = Y0 + (t >> 5), x0 = X0 + PX * (t & 31);
    const bool active = y < a.out_h && x0 < a.out_w;
    int v[PX] = {0, 0, 0, 0};

    // rule 2 on the first n_list entries, highest lane first; a pixel stops at its first hit (rule 3)
    auto resolve = [&](int n_list) {
        if (!active) return;
        for (int e = 0; e < n_list; ++e) {
            if (v[0] && v[1] && v[2] && v[3]) break;
            const int4 s = s_list[e];                                              // the same address in every lane: a broadcast
            const int ax = (short)(s.x & 0xffff), ay = s.x >> 16, bx = (short)(s.y & 0xffff), by = s.y >> 16;
            if (y < min(ay, by) - r || y > max(ay, by) + r || x0 + PX - 1 < min(ax, bx) - r || x0 > max(ax, bx) + r)
                continue;                                                          // no pixel this far from the box is within w / 2
            const int dx = bx - ax, dy = by - ay, L2 = __mul24(dx, dx) + __mul24(dy, dy);
            const long rhs = (long)w2 * L2;
            const int qy = y - ay, ey = y - by;
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                if (v[j]) continue;
                const int qx = x0 + j - ax;
                const int dot = __mul24(qx, dx) + __mul24(qy, dy);
                bool in;
                if (dot <= 0) in = 4 * (__mul24(qx, qx) + __mul24(qy, qy)) <= w2;               // before the first end point
                else if (dot >= L2) { const int ex = x0 + j - bx; in = 4 * (__mul24(ex, ex) + __mul24(ey, ey)) <= w2; }   // past the second
                else { const long c = __mul24(qx, dy) - __mul24(qy, dx); in = 4 * c * c <= rhs; }   // between
                if (in) v[j] = s.z;
            }
        }
    };

    // ---- phase 2: the lanes that passed, highest k first; thread t owns point t ----
    int n_list = 0;
    for (int k = n - 1; k >= 0; --k) {
        if (!s_hit[k]) continue;                                                   // workgroup-uniform
        if (n_list + kMaxOffsets - 1 > kCap) {                                     // the list might not take this lane: flush
            __syncthreads();
            resolve(n_list);
            __syncthreads();
            n_list = 0;
        }
        int val = k + 1;                                                           // rule 4
        if (a.track_id) {
            const int sl = a.slot[(size_t)f * L + k];
            const int id = (unsigned)sl < (unsigned)L ? a.track_id[(size_t)f * L + sl] : 0;
            val = id >= 1 ? 1 + (id - 1) % 254 : 255;
        }
        const int c_raw = cnts[k];
        const int c = c_raw < 0 ? 0 : (c_raw > S ? S : c_raw);
        int px = 0, py = 0;
        const bool ok = t < c && map_point(pts[(size_t)k * S + t], a.sx, a.sy, a.oy, px, py);
        const int mine = (int)(((unsigned)px & 0xffffu) | ((unsigned)py << 16));
        s_pts[t] = mine;
        const unsigned long long m = __ballot(ok);
        if (lane == 0) s_mask[wave] = m;
        __syncthreads();
        // the survivor before this one: in this wavefront, else the last one of the nearest earlier wavefront that has any
        int prev = -1;
        const unsigned long long below = m & ((1ull << lane) - 1ull);
        if (below) prev = wave * 64 + 63 - __builtin_clzll(below);
        else
            for (int w = wave - 1; w >= 0 && prev < 0; --w) {
                const unsigned long long mw = s_mask[w];
                if (mw) prev = w * 64 + 63 - __builtin_clzll(mw);
            }
        bool hit = false;
        int first = 0;
        if (ok && prev >= 0) {
            first = s_pts[prev];
            const int ax = (short)(first & 0xffff), ay = first >> 16;
            hit = min(ax, px) - r <= X1 && max(ax, px) + r >= X0 && min(ay, py) - r <= Y1 && max(ay, py) + r >= Y0;
        }
        const unsigned long long hm = __ballot(hit);
        if (lane == 0) s_hcnt[wave] = __popcll(hm);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) { const int h = s_hcnt[w]; before += w < wave ? h : 0; total += h; }
        if (hit) s_list[n_list + before + __popcll(hm & ((1ull << lane) - 1ull))] = make_int4(first, mine, val, 0);
        n_list += total;                                                           // <= kCap: checked before the lane
    }
    __syncthreads();
    resolve(n_list);
    if (!active) return;                                                           // no barrier follows

    // ---- stores: every pixel of the tile once ----
    if (a.label) {
        uint8_t* row = a.label + ((size_t)f * a.out_h + y) * a.out_w;
        if (WIDE) *reinterpret_cast<uint32_t*>(row + x0) = (unsigned)v[0] | (unsigned)v[1] << 8 | (unsigned)v[2] << 16 | (unsigned)v[3] << 24;
        else
            for (int j = 0; j < PX; ++j)
                if (x0 + j < a.out_w) row[x0 + j] = (uint8_t)v[j];
    }
    if (!a.overlay) return;

    int c[PX][3] = {};                                                             // rule 5: the source pixels as 8-bit RGB (none: black)
    if (FMT != 0) {
        const uint8_t* frame = a.src + (size_t)f * a.frame_stride;                 // a frame spans < 2^31 bytes: 32-bit offsets from here
        const unsigned yrow = (unsigned)y * a.pitch;
        if (FMT == 1) {
            if (WIDE) {
                const uint32_t* p = reinterpret_cast<const uint32_t*>(frame + (yrow + 3u * (unsigned)x0));
                const unsigned w[3] = {p[0], p[1], p[2]};
#pragma unroll
                for (int i = 0; i < 3 * PX; ++i) c[i / 3][i % 3] = byte_of(w[i >> 2], i & 3);
            } else {
                for (int j = 0; j < PX; ++j)
                    if (x0 + j < a.out_w)
                        for (int ch = 0; ch < 3; ++ch) c[j][ch] = frame[yrow + 3u * (unsigned)(x0 + j) + ch];
            }
        } else {
            int Y[PX] = {}, U[PX] = {}, V[PX] = {};
            if (FMT == 2) {                                                        // NV12: chroma row y >> 1, one U,V pair per two columns
                const unsigned crow = a.chroma_offset + (unsigned)(y >> 1) * a.pitch;
                if (WIDE) {
                    const unsigned yw = *reinterpret_cast<const uint32_t*>(frame + (yrow + (unsigned)x0));
                    const unsigned uv = *reinterpret_cast<const uint32_t*>(frame + (crow + (unsigned)x0));     // U0 V0 U1 V1
#pragma unroll
                    for (int j = 0; j < PX; ++j) { Y[j] = byte_of(yw, j); U[j] = byte_of(uv, 2 * (j >> 1)); V[j] = byte_of(uv, 2 * (j >> 1) + 1); }
                } else {
                    for (int j = 0; j < PX; ++j)
                        if (x0 + j < a.out_w) {
                            const unsigned x = (unsigned)(x0 + j);
                            Y[j] = frame[yrow + x]; U[j] = frame[crow + 2 * (x >> 1)]; V[j] = frame[crow + 2 * (x >> 1) + 1];
                        }
                }
            } else {                                                               // YUYV: Y0 U Y1 V per two columns
                if (WIDE) {
                    const uint32_t* p = reinterpret_cast<const uint32_t*>(frame + (yrow + 2u * (unsigned)x0));
                    const unsigned w[2] = {p[0], p[1]};
#pragma unroll
                    for (int j = 0; j < PX; ++j) { Y[j] = byte_of(w[j >> 1], 2 * (j & 1)); U[j] = byte_of(w[j >> 1], 1); V[j] = byte_of(w[j >> 1], 3); }
                } else {
                    for (int j = 0; j < PX; ++j)
                        if (x0 + j < a.out_w) {
                            const unsigned x = (unsigned)(x0 + j);
                            Y[j] = frame[yrow + 2 * x]; U[j] = frame[yrow + 4 * (x >> 1) + 1]; V[j] = frame[yrow + 4 * (x >> 1) + 3];
                        }
                }
            }
#pragma unroll
            for (int j = 0; j < PX; ++j)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) c[j][ch] = csc_channel(a.k, ch, Y[j], U[j], V[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < PX; ++j)
        if (v[j]) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                c[j][ch] = (c[j][ch] * (256 - a.alpha) + (int)s_pal[3 * v[j] + ch] * a.alpha + 128) >> 8;
        }
    uint8_t* orow = a.overlay + (((size_t)f * a.out_h + y) * a.out_w + x0) * 3;
    if (WIDE) {
        unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 3 * PX; ++i) w[i >> 2] |= (unsigned)c[i / 3][i % 3] << (8 * (i & 3));
        uint32_t* o = reinterpret_cast<uint32_t*>(orow);
        o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
    } else {
        for (int j = 0; j < PX; ++j)
            if (x0 + j < a.out_w)
                for (int ch = 0; ch < 3; ++ch) orow[3 * j + ch] = (uint8_t)c[j][ch];
    }
}

inline bool finite_d(double v) { return v == v && v - v == 0.0; }

}  // namespace

// The rules and the arguments: include/phnet_hip.h.
PHNET_API int phnet_lane_draw(const float* points, const int32_t* count, const int32_t* lanes_num, const int32_t* slot,
                              const int32_t* track_id, int64_t F, int32_t L, int32_t S, double sx, double sy, double oy,
                              int32_t out_h, int32_t out_w, int32_t lane_width, const uint8_t* src, int32_t src_format,
                              int64_t frame_stride, int32_t pitch, int64_t chroma_offset, const int32_t* csc_host,
                              const uint8_t* palette, int32_t alpha, uint8_t* label_map, uint8_t* overlay, void* stream)
{
    if (!points || !count || !lanes_num || ((uintptr_t)points & 7)) return PHNET_ERR_ARG;
    if (track_id && !slot) return PHNET_ERR_ARG;
    if (F < 1 || L < 1 || L > kMaxLanes || S < 2 || S > kMaxOffsets) return PHNET_ERR_ARG;
    if (!finite_d(sx) || !finite_d(sy) || !finite_d(oy)) return PHNET_ERR_ARG;
    if (out_h < 1 || out_w < 1 || out_h > 4096 || out_w > 4096 || lane_width < 1 || lane_width > 256 || alpha < 0 || alpha > 256)
        return PHNET_ERR_ARG;
    if (!label_map && !overlay) return PHNET_ERR_ARG;
    if (overlay && !palette) return PHNET_ERR_ARG;
    if (src_format < 0 || src_format > 3) return PHNET_ERR_ARG;
    DrawArgs a{};
    if (src_format != 0) {
        if (!src) return PHNET_ERR_ARG;
        if ((src_format != 1 && (out_w & 1)) || (src_format == 2 && (out_h & 1))) return PHNET_ERR_ARG;       // subsampled chroma
        const int64_t row_bytes = (src_format == 1 ? 3 : src_format == 2 ? 1 : 2) * (int64_t)out_w;
        if (pitch < row_bytes) return PHNET_ERR_ARG;
        if (src_format == 2 && chroma_offset < (int64_t)pitch * out_h) return PHNET_ERR_ARG;
        // the last byte a frame owns: frames closer together than that would overlap
        const int64_t extent = src_format == 2 ? chroma_offset + (int64_t)(out_h / 2 - 1) * pitch + out_w : (int64_t)(out_h - 1) * pitch + row_bytes;
        if (frame_stride < extent || extent >= INT32_MAX) return PHNET_ERR_ARG;
        if (src_format != 1 && (!csc_host || !phnet_csc_from_host(csc_host, a.k))) return PHNET_ERR_ARG;
    }
    const int64_t tiles_x = ceil_div64(out_w, TW), tiles = tiles_x * ceil_div64(out_h, TH);
    if (F > INT32_MAX || F * tiles >= INT32_MAX) return PHNET_ERR_ARG;              // the grid's x dimension
    const int fmt = overlay ? src_format : 0;                                       // a label map alone never reads the source
    a.points = reinterpret_cast<const float2*>(points); a.count = count; a.lanes_num = lanes_num; a.slot = slot; a.track_id = track_id;
    a.L = L; a.S = S; a.sx = sx; a.sy = sy; a.oy = oy; a.out_h = out_h; a.out_w = out_w; a.lane_width = lane_width;
    a.src = src; a.frame_stride = (long)frame_stride; a.pitch = (unsigned)pitch; a.chroma_offset = src_format == 2 ? (unsigned)chroma_offset : 0u;
    a.palette = palette; a.alpha = alpha; a.label = label_map; a.overlay = overlay;
    a.tiles_x = (unsigned)tiles_x; a.tiles_per_frame = (unsigned)tiles;
    // dword stores and loads need every address of them aligned: bases, frame strides, row lengths
    uint64_t low = (uint64_t)(out_w & 3) | (uint64_t)(uintptr_t)label_map | (uint64_t)(uintptr_t)overlay;
    if (fmt != 0) low |= (uint64_t)(uintptr_t)src | (uint64_t)frame_stride | (uint64_t)pitch | (fmt == 2 ? (uint64_t)chroma_offset : 0);
    const bool wide = (low & 3) == 0;
    const dim3 grid((unsigned)(F * tiles));                                        // a workgroup never straddles two frames
#define PHNET_DRAW_LAUNCH(FMT) do {                                                                                                  \
        if (wide) hipLaunchKernelGGL((lane_draw_kernel<FMT, true>), grid, dim3(NT), 0, (hipStream_t)stream, a);                      \
        else hipLaunchKernelGGL((lane_draw_kernel<FMT, false>), grid, dim3(NT), 0, (hipStream_t)stream, a); } while (0)
    switch (fmt) {
        case 0: PHNET_DRAW_LAUNCH(0); break;
        case 1: PHNET_DRAW_LAUNCH(1); break;
        case 2: PHNET_DRAW_LAUNCH(2); break;
        default: PHNET_DRAW_LAUNCH(3); break;
    }
#undef PHNET_DRAW_LAUNCH
    return phnet_launch_status();
}
