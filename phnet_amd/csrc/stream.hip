// Streaming inference: the cross-frame memory of B live video streams as a device-resident token ring (DESIGN.md
// "Streaming path").  One captured hipGraph serves every frame of a video of any length, so nothing here may depend on a
// value the host knows: the ring position is a word in device memory.
//
// State (caller-allocated, device):  ring f32 [S][B][W][L+1][E], ring_valid u8 [S][B][W][L+1]  (S stages, B streams, W =
// save_freq_max slots, L = max_lanes, E = token width);  n i32[B] = frames pushed since the stream's last reset (a reset is the
// host writing n[b] = 0, stream-ordered; validity follows from n, the ring is never cleared);  cursor i32[B] = the copy of n
// that phnet_stream_window publishes for phnet_stream_push.
//
// Read / advance hazard: every workgroup of a launch reads the frame counter, so no launch may write the word it reads (a late
// workgroup would see the advanced value).  window READS n and one thread WRITES cursor;  push READS cursor and one thread
// WRITES n = cursor + 1.  Per frame: window, ..., push.  A push that is repeated without a window in between rewrites the same
// slot and leaves n unchanged.
#include "common.h"

namespace {

// Logical slot j (0 = oldest remembered frame) of a stream that has pushed n frames lives in physical slot (n - c + j) % W,
// c = min(n, W); slots j >= c are empty.  (stream.py window_order is the same statement in Python.)
__device__ __forceinline__ int physical_slot(int n, int W, int j) { return (n - min(n, W) + j) % W; }

// Memory entry of one (stage, stream) = memory_tokens_kernel (elementwise.hip) with the SAME summation order (groups of
// blockDim.x / E threads stride the anchors, partials folded in group order, the positives subtracted in prior order), written
// to slot cursor % W of the ring.  blockIdx.x = stream b, blockIdx.y = stage s.  The positives' rows are fetched by the
// thread groups in parallel BEFORE the anchor sum (one group per lane; their loads overlap the sum's), then folded by group 0.
__global__ __launch_bounds__(1024) void stream_push_kernel(const float* __restrict__ feat, const long long* __restrict__ rows,
                                                           float* __restrict__ ring, unsigned char* __restrict__ ring_valid,
                                                           const int* __restrict__ cursor, int* __restrict__ n_out,
                                                           int B, int W, int N, int E, int L)
{
    extern __shared__ float lds[];                   // part [groups][E], then pos [L][E]
    const int b = blockIdx.x, s = blockIdx.y;
    const int e = threadIdx.x % E, grp = threadIdx.x / E, groups = blockDim.x / E;
    const int n = max(cursor[b], 0);
    const int slot = n % W;
    feat += ((size_t)s * B + b) * N * E;
    rows += (size_t)b * L;
    float* tokens = ring + (((size_t)s * B + b) * W + slot) * (size_t)(L + 1) * E;
    unsigned char* valid = ring_valid + (((size_t)s * B + b) * W + slot) * (size_t)(L + 1);
    float* part = lds;
    float* pos = lds + (size_t)groups * E;
    for (int l = grp; l < L; l += groups) {
        const long long r = rows[l];
        const bool ok = r >= 0 && r < N;
        const float v = ok ? feat[(size_t)r * E + e] : 0.f;
        tokens[(size_t)l * E + e] = v;
        pos[l * E + e] = v;
        if (e == 0) valid[l] = ok;
    }
    float sum = 0.f;
    for (int a = grp; a < N; a += groups) sum += feat[(size_t)a * E + e];
    part[grp * E + e] = sum;
    __syncthreads();
    if (grp != 0) return;
    float total = 0.f;
    for (int g2 = 0; g2 < groups; ++g2) total += part[g2 * E + e];
    float possum = 0.f;
    int cnt = 0;
    for (int l = 0; l < L; ++l) {
        const long long r = rows[l];
        possum += pos[l * E + e];
        cnt += r >= 0 && r < N;
    }
    tokens[(size_t)L * E + e] = (total - possum) / (float)(N - cnt);
    if (e == 0) {
        valid[L] = 1;
        // the only write of n in this launch; nobody in it reads n.  Beyond 2^30 frames the count is folded by a multiple of W:
        // same slot, still >= W, no overflow
        if (s == 0) n_out[b] = n + 1 < (1 << 30) ? n + 1 : n + 1 - ((1 << 30) / W - 1) * W;
    }
}

// The memory the next frame attends to, in logical order: blockIdx.x = logical slot j, blockIdx.y = stream, blockIdx.z = stage.
// Filled slots are copied from the ring (16-byte moves), empty ones are written as zeros and marked invalid.
__global__ __launch_bounds__(256) void stream_window_kernel(const float* __restrict__ ring, const unsigned char* __restrict__ ring_valid,
                                                            const int* __restrict__ n_in, int* __restrict__ cursor,
                                                            float* __restrict__ window, unsigned char* __restrict__ window_valid,
                                                            unsigned char* __restrict__ has_memory, int B, int W, int L1, int E)
{
    const int j = blockIdx.x, b = blockIdx.y, s = blockIdx.z;
    const int n = n_in[b];
    const bool filled = j < min(n, W);
    const size_t sb = (size_t)s * B + b;
    const int row4 = L1 * E / 4;                     // E % 4 == 0
    const float4* src = reinterpret_cast<const float4*>(ring + (sb * W + (filled ? physical_slot(n, W, j) : 0)) * (size_t)L1 * E);
    float4* dst = reinterpret_cast<float4*>(window + (sb * W + j) * (size_t)L1 * E);
    for (int i = threadIdx.x; i < row4; i += blockDim.x) dst[i] = filled ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const unsigned char* vsrc = ring_valid + (sb * W + (filled ? physical_slot(n, W, j) : 0)) * (size_t)L1;
    for (int i = threadIdx.x; i < L1; i += blockDim.x) window_valid[(sb * W + j) * (size_t)L1 + i] = filled ? vsrc[i] : 0;
    if (j == 0 && s == 0 && threadIdx.x == 0) {
        has_memory[b] = n > 0;
        cursor[b] = n;                               // the only write of cursor in this launch; nobody in it reads cursor
    }
}

// feat[b] = attn[b] for the streams whose memory is empty (the reference skips the cross-frame decoder there,
// Router4OL.py:349-353); streams with a memory keep the decoder's rows untouched.  per4 = float4 elements per stream.
__global__ __launch_bounds__(256) void stream_select_kernel(const float* __restrict__ attn, const unsigned char* __restrict__ has_memory,
                                                            float* __restrict__ feat, int per4)
{
    const int b = blockIdx.y;
    if (has_memory[b]) return;
    const float4* src = reinterpret_cast<const float4*>(attn) + (size_t)b * per4;
    float4* dst = reinterpret_cast<float4*>(feat) + (size_t)b * per4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < per4; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

}  // namespace

// feat [S][B][N][E] (this frame's cat(local, pos) of every stage), anchors_sorted i64[B][L] (kept anchors ascending, -1 padded).
PHNET_API int phnet_stream_push(const float* feat, const int64_t* anchors_sorted, float* ring, uint8_t* ring_valid,
                                const int32_t* cursor, int32_t* n, int32_t S, int32_t B, int32_t W, int32_t N, int32_t E, int32_t L,
                                void* stream)
{
    if (S < 1 || S > 65535 || B < 1 || W < 1 || N < 1 || E < 1 || E > 1024 || L < 1 || L >= N || !feat || !anchors_sorted || !ring || !ring_valid ||
        !cursor || !n)
        return PHNET_ERR_ARG;
    const int groups = 1024 / E;                     // as phnet_memory_tokens: the summation order depends on it
    const size_t lds = (size_t)(groups + L) * E * sizeof(float);
    if (lds > 64 * 1024) return PHNET_ERR_ARG;
    hipLaunchKernelGGL(stream_push_kernel, dim3(B, S), dim3(groups * E), lds, (hipStream_t)stream, feat,
                       (const long long*)anchors_sorted, ring, ring_valid, cursor, n, B, W, N, E, L);
    return phnet_launch_status();
}

// window [S][B][W*(L+1)][E], window_valid u8 [S][B][W*(L+1)], has_memory u8[B].
PHNET_API int phnet_stream_window(const float* ring, const uint8_t* ring_valid, const int32_t* n, int32_t* cursor, float* window,
                                  uint8_t* window_valid, uint8_t* has_memory, int32_t S, int32_t B, int32_t W, int32_t E, int32_t L,
                                  void* stream)
{
    if (S < 1 || B < 1 || W < 1 || E < 1 || E % 4 || L < 1 || S > 65535 || B > 65535 || !ring || !ring_valid || !n || !cursor ||
        !window || !window_valid || !has_memory)
        return PHNET_ERR_ARG;
    hipLaunchKernelGGL(stream_window_kernel, dim3(W, B, S), dim3(256), 0, (hipStream_t)stream, ring, ring_valid, n, cursor, window,
                       window_valid, has_memory, B, W, L + 1, E);
    return phnet_launch_status();
}

// attn, feat [B][N][E]; has_memory u8[B].  In place on feat (the decoder's output).
PHNET_API int phnet_stream_select(const float* attn, const uint8_t* has_memory, float* feat, int32_t B, int32_t N, int32_t E,
                                  void* stream)
{
    if (B < 1 || B > 65535 || N < 1 || E < 1 || E % 4 || !attn || !has_memory || !feat) return PHNET_ERR_ARG;
    const int per4 = (int)((int64_t)N * E / 4);
    const int64_t blocks = ceil_div64(per4, 256);
    hipLaunchKernelGGL(stream_select_kernel, dim3((unsigned)(blocks < 64 ? blocks : 64), B), dim3(256), 0, (hipStream_t)stream, attn,
                       has_memory, feat, per4);
    return phnet_launch_status();
}
