// Internal (not part of the C-ABI): what csrc/linrows.hip takes from csrc/conv.hip, so that the split of a reduction and the reduce
// launch are stated once.
#pragma once
#include "common.h"

struct ConvSplit { int splits, k_per_split; };

// Split-K factor and K range per split that phnet_conv2d_fwd (dgrad = false: x [M][K], w [N][K]) or phnet_conv2d_dgrad (dgrad = true:
// dy [M][K], w [K][N]) runs the Linear layer M x N, reduction depth K, with - pick_conv's answer for the current tuning state.
ConvSplit phnet_linear_split(long M, int K, int N, bool dgrad, bool has_ws, size_t ws_bytes);

// out [M][N] = sum of the `splits` slabs of `part` (+ bias) (ReLU): the splitk_reduce_kernel launch of launch_conv
void phnet_splitk_reduce(const float* part, float* out, const float* bias, long M, int N, int splits, int relu, hipStream_t st);
