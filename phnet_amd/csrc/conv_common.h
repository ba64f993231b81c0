// Shapes and small helpers shared by the implicit-GEMM sources: conv.hip (forward / data gradient), conv_wgrad.hip (weight
// gradient) and linear_bwd.hip (fused few-rows Linear backward, and conv.hip's kernels of arithmetic modes 0 / 1 / 2).  Internal, not part of the C-ABI.
// All of it sits in the unnamed namespace: the kernels take ConvShape / WgradShape by value and their symbols spell them that way.
#pragma once
#include <type_traits>
#include "igemm.h"
static constexpr bool g_interleave = true;                   // MFMA / VALU interleave hints of the staged-split loops

namespace {

struct ConvShape {
    int N, Hi, Wi, Ci;       // A-side image (input for fwd, dY for dgrad)
    int Ho, Wo, Co;          // GEMM output image
    int R, S;
    int stride, pad, in_dil; // coordinate: t = o*stride - pad + r ; valid iff t % in_dil == 0 ; i = t / in_dil
    int splits;              // split-K factor (blockIdx.z)
    int k_per_split;         // multiple of BK
};

struct RowCoord { int base, iy0, ix0; bool ok; };

// f(integral_constant<0>, t), f(integral_constant<1>, t + 1), ... : a loop body that needs its index at compile time
template <int N, int I = 0, typename F>
__device__ __forceinline__ void unroll_iterations(F& f, int t) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{}, t + I);
        unroll_iterations<N, I + 1>(f, t);
    }
}
template <int N, int I = 0, typename F>
__device__ __forceinline__ void tail_iterations(F& f, int t, int end) {
    if constexpr (I < N) {
        if (t + I < end) {
            f(std::integral_constant<int, I>{}, t + I);
            tail_iterations<N, I + 1>(f, t, end);
        }
    }
}

struct WgradShape {
    int N, Hi, Wi, Ci;       // forward input image X
    int Ho, Wo, Co;          // forward output image (dY)
    int R, S, stride, pad;
    int splits, pix_per_split;   // multiple of BK
};

bool conv_args_ok(int N, int Hi, int Wi, int Ci, int Co, int R, int S, int stride, int pad)
{
    return !(N < 0 || Hi < 1 || Wi < 1 || Ci < 4 || Co < 4 || (Ci & 3) || (Co & 3) || R < 1 || S < 1 || stride < 1 || pad < 0);
}

// GEMM view of the forward; false where the output image would be empty
bool fwd_shape(int N, int Hi, int Wi, int Ci, int Co, int R, int S, int stride, int pad, ConvShape* g)
{
    *g = ConvShape{};
    g->N = N; g->Hi = Hi; g->Wi = Wi; g->Ci = Ci; g->Co = Co; g->R = R; g->S = S;
    g->Ho = (Hi + 2 * pad - R) / stride + 1;
    g->Wo = (Wi + 2 * pad - S) / stride + 1;
    g->stride = stride; g->pad = pad; g->in_dil = 1;
    return g->Ho >= 1 && g->Wo >= 1;
}

// GEMM view of the data gradient (A side = dY, output = dX); false for paddings it does not support
bool dgrad_shape(int N, int Hi, int Wi, int Ci, int Co, int R, int S, int stride, int pad, ConvShape* g)
{
    *g = ConvShape{};
    g->N = N;
    g->Hi = (Hi + 2 * pad - R) / stride + 1;      // A-side image = dY
    g->Wi = (Wi + 2 * pad - S) / stride + 1;
    g->Ci = Co;
    g->Ho = Hi; g->Wo = Wi; g->Co = Ci;            // GEMM output = dX
    g->R = R; g->S = S;
    g->stride = 1; g->pad = R - 1 - pad; g->in_dil = stride;
    if (R != S && (S - 1 - pad) != g->pad) return false;        // square padding only
    return g->pad >= 0;
}

static bool wgrad_shape(int N, int Hi, int Wi, int Ci, int Co, int R, int S, int stride, int pad, WgradShape* g)
{
    *g = WgradShape{};
    g->N = N; g->Hi = Hi; g->Wi = Wi; g->Ci = Ci; g->Co = Co; g->R = R; g->S = S; g->stride = stride; g->pad = pad;
    g->Ho = (Hi + 2 * pad - R) / stride + 1;
    g->Wo = (Wi + 2 * pad - S) / stride + 1;
    return conv_args_ok(N, Hi, Wi, Ci, Co, R, S, stride, pad);
}

}  // namespace
