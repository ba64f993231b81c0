// Streaming inference of the Router4OLV2 family: the key set the cross-frame decoder of one refinement stage attends to, for B
// live streams under one captured hipGraph (DESIGN.md "Streaming path", V2 rules).
//
// The V2 head differs from V1 (csrc/stream.hip) in two ways that only the device can decide once the step is captured:
//   * a frame without a usable memory does NOT skip the decoder, it attends to its OWN N tokens (Router4OLV2.py:320-325);
//   * the memory is used from frame `save_freq` on, although the ring is pushed from frame 0 - so "has a ring entry" (n > 0) is
//     the wrong test, the frame count since the reset decides.
// Both are answered per stream by cursor[b], the copy of the frame count that phnet_stream_window published for this step.  This
// launch reads cursor and never n: no launch reads a word that a launch of the same step advances (stream.hip, header comment).
//
// The key set has the fixed size Kmax >= max(N, M) (M = W * (L + 1) window rows): valid keys first at unchanged positions, masked
// ones after - the attention kernel deals keys round-robin to the lanes of a row and skips masked ones, so the padded set gives
// the bits of the clip path's exact-size key set (stream.py window_order).
#include "common.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));     // native 16-byte vector: selects between rows stay in registers

constexpr int kThreads = 256;
constexpr int kRowsPerBlock = 8;     // E = 256: 8 rows x 64 float4 = two rounds of the 256 threads; Kmax = 240 -> grid 30 x B

// blockIdx.x = block of kRowsPerBlock key rows, blockIdx.y = stream.  Row r < N: tgt = local + pos (one add per element), written
// where phnet_stream_push reads it.  Key row r: the stream's window row (r < M) when its memory is in use, its own tgt row (r < N)
// otherwise, zeros / invalid beyond.  16-byte loads and stores; e4 = E / 4.
__global__ __launch_bounds__(kThreads) void stream_keys_kernel(const f4* __restrict__ local, const f4* __restrict__ pos,
                                                               const f4* __restrict__ window,
                                                               const unsigned char* __restrict__ window_valid,
                                                               const int* __restrict__ cursor, f4* __restrict__ tgt,
                                                               f4* __restrict__ keys, unsigned char* __restrict__ keys_valid,
                                                               int N, int M, int Kmax, int e4, int min_frames)
{
    const int b = blockIdx.y;
    const int c = cursor[b];
    // an empty memory is never a key set (min_frames = 0, first frame: the reference falls back on `shape[0] == 0` as well)
    const bool use_mem = c >= min_frames && c > 0;
    const int r0 = blockIdx.x * kRowsPerBlock;
    const int rows = min(kRowsPerBlock, Kmax - r0);
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < rows * e4; i += kThreads) {
        const int r = r0 + i / e4, e = i % e4;
        f4 t = zero;
        if (r < N) {
            t = local[((size_t)b * N + r) * e4 + e] + pos[(size_t)r * e4 + e];
            tgt[((size_t)b * N + r) * e4 + e] = t;
        }
        f4 k = t;                                     // own token (zero beyond N)
        if (use_mem) {
            k = zero;
            if (r < M) k = window[((size_t)b * M + r) * e4 + e];
        }
        keys[((size_t)b * Kmax + r) * e4 + e] = k;
        if (e == 0) keys_valid[(size_t)b * Kmax + r] = use_mem ? (r < M ? (window_valid[(size_t)b * M + r] != 0) : 0) : (r < N);
    }
}

}  // namespace

// local, tgt [B][N][E]; pos [N][E]; window [B][M][E], window_valid u8 [B][M] (one stage of what phnet_stream_window wrote);
// cursor i32[B]; keys [B][Kmax][E], keys_valid u8 [B][Kmax].
PHNET_API int phnet_stream_keys(const float* local, const float* pos, const float* window, const uint8_t* window_valid,
                                const int32_t* cursor, float* tgt, float* keys, uint8_t* keys_valid, int32_t B, int32_t N, int32_t M,
                                int32_t Kmax, int32_t E, int32_t min_frames, void* stream)
{
    if (B < 1 || B > 65535 || N < 1 || M < 1 || E < 4 || E % 4 || Kmax < N || Kmax < M || min_frames < 0 || !local || !pos || !window ||
        !window_valid || !cursor || !tgt || !keys || !keys_valid)
        return PHNET_ERR_ARG;
    const int64_t blocks = ceil_div64(Kmax, kRowsPerBlock);
    if (blocks > 0x7fffffff) return PHNET_ERR_ARG;
    hipLaunchKernelGGL(stream_keys_kernel, dim3((unsigned)blocks, B), dim3(kThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const f4*>(local), reinterpret_cast<const f4*>(pos), reinterpret_cast<const f4*>(window),
                       window_valid, cursor, reinterpret_cast<f4*>(tgt), reinterpret_cast<f4*>(keys), keys_valid, N, M, Kmax, E / 4,
                       min_frames);
    return phnet_launch_status();
}
