// Mask-level video metrics on the device: the seven integer counts per frame behind region similarity J and boundary F-measure F
// (DESIGN.md "Mask metrics"; the numbered rules are in include/phnet_hip.h).  Replaces the host work of the reference's
// evaluation/evaluate_vid.py:51-57 with video_metrics/jaccard.py and f_boundary.py (seg2bmap, two skimage binary_dilation calls
// with disk(ceil(0.008 diagonal)) and five np.sum per frame pair) for label maps that are already on the device.
//
// Everything is integer and bit arithmetic: a mask row is 64-pixel words (one __ballot per word), a boundary map is a sparse bit
// image, the disk dilation is shifts and ORs of those words, the counts are popcounts.  No floating point anywhere.
//
// Pass one (mask_boundary_kernel): a wavefront owns one 64-pixel column of words and walks kRows1 rows downwards, one pixel per
//   lane.  Two ballots per mask and row give the foreground word F and the bit of the pixel right of the word; with the row below
//   (F', read once and kept for the next step) the boundary word of rule 2 is
//       b = ((F ^ Fe) & Me) | (F ^ F') | ((F ^ Fe') & Me)      Fe = F one pixel to the left, Me = the columns x < W - 1,
//   the last row keeps the first term only.  Ballots and everything after them are wave-uniform, so this is scalar work.  Every
//   word of the workspace [n][2][H][ceil(W / 64)] is stored, bits past W are zero; areas and boundary sizes leave as five integer
//   atomics per workgroup.
// Pass two (mask_match_kernel): a workgroup owns a tile of kTileRows x kTileWords words of A (the boundary whose pixels are
//   counted) in one frame and one direction (A = b_pred against dil(b_gt): fg_match; A = b_gt against dil(b_pred): gt_match).
//   Non-zero words of A are few: they are collected into a list first, and a tile without any ends there.  Otherwise the words of
//   B under the tile and `radius` rows / ceil(radius / 64) words around it go to LDS (zero outside the image: rule 3), and every
//   thread takes list entries: for dy = -radius .. radius it reads the 2 K + 1 words of row y + dy around its word, skips the row
//   when they are all zero (most are), else ORs their horizontal dilation by hw(dy) = isqrt(radius^2 - dy^2) into its accumulator
//   and stops as soon as every pixel of A's word is covered.  popcount(A & acc) goes to an LDS counter, one atomic per tile to
//   global memory.
// Integer sums do not depend on their order: the counts are bit-reproducible whatever the schedule.  The counts are zeroed by a
// memset node in front of pass one, so nothing depends on what `counts` or the workspace held.
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int kMaxRadius = 127, kMaxSize = 4096;              // PHNET_MASK_METRICS_MAX_RADIUS / _MAX_SIZE of the public header
constexpr int NT = 256;
constexpr int kRows1 = 64;                                    // pass one: rows of a wavefront
constexpr int kTileRows = 32, kTileWords = 8;                 // pass two: the tile of a workgroup, kTileRows * kTileWords = NT words
constexpr int kMaxHaloWords = (kMaxRadius + 63) / 64;         // 2
constexpr int kWin = 2 * kMaxHaloWords + 1;                   // 5 words: the target word and 128 pixels to either side
constexpr int kLdsWords = (kTileRows + 2 * kMaxRadius) * (kTileWords + 2 * kMaxHaloWords);     // 286 * 12 words = 27456 bytes
static_assert(kTileRows * kTileWords == NT, "one tile word per thread");

struct Row { u64 f, fe; };                                    // foreground of a word; the same one pixel to the left (bit i = pixel i + 1)

// the word of pixels x0 .. x0 + 63 of `row` (W pixels) for the whole wavefront; `x` = x0 + lane.  Pixels past W read as background.
__device__ __forceinline__ Row load_row(const uint8_t* __restrict__ row, int x, int lane, int W)
{
    const bool fg = x < W && row[x] != 0;                                        // rule 1
    const bool right = lane == 0 && x + 64 < W && row[x + 64] != 0;             // the first pixel of the next word
    const u64 f = __ballot(fg);
    return Row{f, (f >> 1) | (__ballot(right) << 63)};
}

__device__ __forceinline__ void atomic_add64(int64_t* p, u64 v) { atomicAdd(reinterpret_cast<u64*>(p), v); }

__global__ __launch_bounds__(NT) void mask_boundary_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, int H, int W,
                                                           int WW, unsigned chunks_y, unsigned groups_x, u64* __restrict__ bmaps,
                                                           int64_t* __restrict__ counts)
{
    __shared__ unsigned s_cnt[5];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned b = blockIdx.x;
    const unsigned gx = b % groups_x; b /= groups_x;
    const unsigned cy = b % chunks_y;
    const unsigned f = b / chunks_y;
    if (t < 5) s_cnt[t] = 0u;
    __syncthreads();

    const int w = (int)gx * (NT / 64) + wave;                                      // this wavefront's word column
    if (w < WW) {                                                                  // wave-uniform
        const int x = w * 64 + lane;
        const int ne = min(64, W - 1 - w * 64);                                    // columns of the word left of the image's last column
        const u64 Me = ne >= 64 ? ~0ull : ne <= 0 ? 0ull : (1ull << ne) - 1ull;
        const size_t frame = (size_t)f * H * W;
        const uint8_t* P = pred + frame;
        const uint8_t* G = gt + frame;
        u64* outP = bmaps + ((size_t)f * 2 + 0) * H * WW + w;
        u64* outG = bmaps + ((size_t)f * 2 + 1) * H * WW + w;
        const int y0 = (int)cy * kRows1, y1 = min(y0 + kRows1, H);
        unsigned aP = 0, aG = 0, aB = 0, nP = 0, nG = 0;                            // <= 64 * 64 each
        Row p = load_row(P + (size_t)y0 * W, x, lane, W), g = load_row(G + (size_t)y0 * W, x, lane, W);
        for (int y = y0; y < y1; ++y) {
            u64 bp = (p.f ^ p.fe) & Me, bg = (g.f ^ g.fe) & Me;                    // rule 2, the last row's form
            aP += __popcll(p.f); aG += __popcll(g.f); aB += __popcll(p.f & g.f);
            if (y + 1 < H) {
                const Row p2 = load_row(P + (size_t)(y + 1) * W, x, lane, W), g2 = load_row(G + (size_t)(y + 1) * W, x, lane, W);
                bp |= (p.f ^ p2.f) | ((p.f ^ p2.fe) & Me);
                bg |= (g.f ^ g2.f) | ((g.f ^ g2.fe) & Me);
                p = p2; g = g2;
            }
            nP += __popcll(bp); nG += __popcll(bg);
            if (lane == 0) { outP[(size_t)y * WW] = bp; outG[(size_t)y * WW] = bg; }
        }
        if (lane == 0) {
            atomicAdd(&s_cnt[0], aP); atomicAdd(&s_cnt[1], aG); atomicAdd(&s_cnt[2], aB); atomicAdd(&s_cnt[3], nP); atomicAdd(&s_cnt[4], nG);
        }
    }
    __syncthreads();
    if (t < 5 && s_cnt[t]) atomic_add64(counts + (size_t)f * 7 + t, s_cnt[t]);
}

// d |= d >> (64 Q + b), 0 <= b < 64, on the kWin-word integer d (word 0 lowest; zero above word kWin - 1).  Ascending j reads only
// words that have not been updated yet.
template <int Q>
__device__ __forceinline__ void or_shr_words(u64 (&d)[kWin], int b)
{
#pragma unroll
    for (int j = 0; j + Q < kWin; ++j) {
        const u64 lo = d[j + Q], hi = j + Q + 1 < kWin ? d[j + Q + 1] : 0ull;
        d[j] |= (lo >> b) | ((hi << 1) << (63 - b));                               // (hi << (64 - b)) without the undefined b = 0
    }
}
__device__ __forceinline__ void or_shr(u64 (&d)[kWin], int s)                      // 0 <= s <= 128, the same in every lane
{
    const int q = s >> 6, b = s & 63;
    if (q == 0) or_shr_words<0>(d, b);
    else if (q == 1) or_shr_words<1>(d, b);
    else or_shr_words<2>(d, b);
}

// The window d holds pixels x0 - 128 .. x0 + 191 of a row (bit p of the integer = pixel x0 - 128 + p).  -> the 64 pixels x0 .. x0 + 63
// of the row dilated horizontally by hw <= 127: pixel i is set iff a pixel in [i - hw, i + hw] is.
// Y = OR of d >> e for e = 0 .. 2 hw has bit p = OR of the bits p .. p + 2 hw of d, so the answer is Y's bits from 128 - hw on.  Y is
// built by doubling: shifts 0 .. span - 1 are in hand, OR-ing a copy `span` lower doubles the run; the last step takes what is left.
__device__ __forceinline__ u64 dilate_row(u64 (&d)[kWin], int hw)
{
    const int n = 2 * hw + 1;                                                      // shifts to cover, 1 .. 255
    int span = 1;
    while (2 * span <= n) { or_shr(d, span); span *= 2; }
    if (n > span) or_shr(d, n - span);
    // bits off .. off + 63 of Y, off = 128 - hw in 1 .. 128 (128: hw = 0, the word itself).  Selects between values, not a switch over off >> 6: the
    // switch's default came back as d[3] on gfx950 (hipcc -O3), which lost every row at dy = +-radius.
    const int off = 128 - hw, q = off >> 6, b = off & 63;
    const u64 r0 = (d[0] >> b) | ((d[1] << 1) << (63 - b)), r1 = (d[1] >> b) | ((d[2] << 1) << (63 - b));
    return q == 0 ? r0 : q == 1 ? r1 : d[2];
}

__device__ __forceinline__ int isqrt_i(int v)                                      // floor(sqrt(v)), 0 <= v <= 127^2; integers only
{
    int r = 0;
#pragma unroll
    for (int bit = 64; bit > 0; bit >>= 1)
        if ((r + bit) * (r + bit) <= v) r += bit;
    return r;
}

__global__ __launch_bounds__(NT) void mask_match_kernel(const u64* __restrict__ bmaps, int H, int WW, int radius, unsigned tiles_y,
                                                        unsigned tiles_x, int64_t* __restrict__ counts)
{
    __shared__ u64 s_b[kLdsWords];                    // B under the tile and its halo, row-major, `stride` words per row
    __shared__ u64 s_a[NT];                           // the non-zero words of A ...
    __shared__ int s_pos[NT];                         // ... and where they are: (row in tile) << 8 | word in tile
    __shared__ int s_n;
    __shared__ unsigned s_sum;

    const int t = threadIdx.x;
    unsigned b = blockIdx.x;
    const unsigned tx = b % tiles_x; b /= tiles_x;
    const unsigned ty = b % tiles_y; b /= tiles_y;
    const unsigned dir = b & 1u, f = b >> 1;
    const int Y0 = (int)ty * kTileRows, W0 = (int)tx * kTileWords;
    const size_t plane = (size_t)H * WW;
    const u64* A = bmaps + ((size_t)f * 2 + dir) * plane;                          // dir 0: b_pred inside dil(b_gt) = fg_match
    const u64* B = bmaps + ((size_t)f * 2 + (dir ^ 1u)) * plane;

    if (t == 0) { s_n = 0; s_sum = 0u; }
    __syncthreads();
    {
        const int ry = t / kTileWords, rw = t % kTileWords, y = Y0 + ry, w = W0 + rw;
        const u64 a = y < H && w < WW ? A[(size_t)y * WW + w] : 0ull;
        if (a) {
            const int k = atomicAdd(&s_n, 1);                                      // < NT: one word per thread.  The order is free: sums
            s_a[k] = a; s_pos[k] = ry << 8 | rw;
        }
    }
    __syncthreads();
    const int n_list = s_n;
    if (n_list == 0) return;                                                       // workgroup-uniform; no barrier follows it for this tile

    const int K = (radius + 63) >> 6;                                              // halo words, 0 .. 2
    const int stride = kTileWords + 2 * K, rows = kTileRows + 2 * radius;          // rows * stride <= kLdsWords
    for (int i = t; i < rows * stride; i += NT) {
        const int lr = i / stride, lc = i - lr * stride;
        const int y = Y0 - radius + lr, w = W0 - K + lc;
        s_b[i] = y >= 0 && y < H && w >= 0 && w < WW ? B[(size_t)y * WW + w] : 0ull;      // rule 3: outside the image nothing is set
    }
    __syncthreads();

    const int r2 = radius * radius;
    unsigned mine = 0;
    for (int e = t; e < n_list; e += NT) {
        const u64 a = s_a[e];
        const int ry = s_pos[e] >> 8, rw = s_pos[e] & 255;
        const u64* centre = s_b + (ry + radius) * stride + rw + K;                 // B's word under A's
        u64 acc = 0;
        for (int dy = -radius; dy <= radius; ++dy) {
            const u64* row = centre + dy * stride;                                 // rows ry .. ry + 2 radius of the staged block
            u64 d[kWin];
            d[2] = row[0];
            d[1] = K >= 1 ? row[-1] : 0ull; d[3] = K >= 1 ? row[1] : 0ull;
            d[0] = K >= 2 ? row[-2] : 0ull; d[4] = K >= 2 ? row[2] : 0ull;
            if (!(d[0] | d[1] | d[2] | d[3] | d[4])) continue;
            acc |= dilate_row(d, isqrt_i(r2 - dy * dy));
            if (!(a & ~acc)) break;                                                // every pixel of this word has found its match
        }
        mine += __popcll(a & acc);
    }
    if (mine) atomicAdd(&s_sum, mine);
    __syncthreads();
    if (t == 0 && s_sum) atomic_add64(counts + (size_t)f * 7 + 5 + dir, s_sum);
}

inline int64_t words_of(int width) { return (width + 63) / 64; }

}  // namespace

// The rules and the arguments: include/phnet_hip.h.
PHNET_API uint64_t phnet_mask_metrics_workspace(int32_t n_frames, int32_t height, int32_t width, int32_t radius)
{
    if (n_frames < 0 || height < 1 || width < 1 || height > kMaxSize || width > kMaxSize || radius < 0 || radius > kMaxRadius) return 0;
    return (uint64_t)n_frames * 2u * (uint64_t)height * (uint64_t)words_of(width) * sizeof(u64);
}

PHNET_API int phnet_mask_metrics(const uint8_t* pred, const uint8_t* gt, int32_t n_frames, int32_t height, int32_t width, int32_t radius,
                                 void* workspace, uint64_t workspace_bytes, int64_t* counts, void* stream)
{
    if (n_frames < 0 || height < 1 || width < 1 || height > kMaxSize || width > kMaxSize || radius < 0 || radius > kMaxRadius)
        return PHNET_ERR_ARG;
    if (n_frames == 0) return PHNET_OK;
    if (!pred || !gt || !counts || !workspace || ((uintptr_t)workspace & 7) || ((uintptr_t)counts & 7)) return PHNET_ERR_ARG;
    if (workspace_bytes < phnet_mask_metrics_workspace(n_frames, height, width, radius)) return PHNET_ERR_ARG;
    const int64_t WW = words_of(width);
    const int64_t chunks_y = ceil_div64(height, kRows1), groups_x = ceil_div64(WW, NT / 64);
    const int64_t tiles_y = ceil_div64(height, kTileRows), tiles_x = ceil_div64(WW, kTileWords);
    const int64_t grid1 = (int64_t)n_frames * chunks_y * groups_x, grid2 = (int64_t)n_frames * 2 * tiles_y * tiles_x;
    if (grid1 >= INT32_MAX || grid2 >= INT32_MAX) return PHNET_ERR_ARG;           // the grid's x dimension
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)n_frames * 7 * sizeof(int64_t), s) != hipSuccess) { (void)hipGetLastError(); return PHNET_ERR_LAUNCH; }
    u64* bmaps = static_cast<u64*>(workspace);
    hipLaunchKernelGGL(mask_boundary_kernel, dim3((unsigned)grid1), dim3(NT), 0, s, pred, gt, (int)height, (int)width, (int)WW,
                       (unsigned)chunks_y, (unsigned)groups_x, bmaps, counts);
    hipLaunchKernelGGL(mask_match_kernel, dim3((unsigned)grid2), dim3(NT), 0, s, (const u64*)bmaps, (int)height, (int)WW, (int)radius,
                       (unsigned)tiles_y, (unsigned)tiles_x, counts);
    return phnet_launch_status();
}
