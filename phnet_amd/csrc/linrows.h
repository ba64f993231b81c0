// Internal (not part of the C-ABI): what csrc/conv.hip takes from csrc/linrows.hip.  pick_conv asks linrows_wm once it has the plan,
// launch_conv launches through linrows_launch (the split of K and the reduce launch stay conv.hip's own), conv_kernel_name spells
// LINROWS_NAME.
#pragma once
#include "common.h"

// linrows_kernel<dgrad, wm>, as rocprofv3 spells it: printf format of ("false" | "true", wm)
constexpr const char* LINROWS_NAME = "linrows_kernel<%s, %d>";
// linrows_bf16_kernel<wm>: its forward in arithmetic mode 4
constexpr const char* LINROWS_BF16_NAME = "linrows_bf16_kernel<%d>";

// The WM (1: 160-row tiles, 2: 320-row tiles) of the linrows_kernel<DGRAD, WM> that takes the Linear layer of M rows, N columns and
// reduction depth K which the plan cuts into `splits` - or 0: it stays on the generic kernel.  Reads tuning().linrows (0: never,
// 1: the shape class measured faster, 2: whatever the kernel can run) and the arithmetic mode: 3, or 4 for a forward (then the launch
// is linrows_bf16_kernel<WM>).
int linrows_wm(bool dgrad, long M, int K, int N, int splits);

// The GEMM launch alone: dst [splits][M][N] (the output itself where splits == 1, with bias and ReLU; else the raw partial sums) from
// a [M][K] and w ([N][K] forward, [K][N] data gradient).  k_per_split: a multiple of 16.  false: the launch could not be set up.
bool linrows_launch(bool dgrad, int wm, const float* a, const float* w, const float* bias, float* dst, long M, int K, int N, int splits,
                    int k_per_split, int relu, hipStream_t st);
