/* Benchmark and A/B switches of libphnet_hip.so - NOT part of the drop-in boundary (include/phnet_hip.h).
 *
 * Process-global (one struct, csrc/tuning.h), not thread-safe, never called by the product path: tests/ and tests/tools/ use them to run one kernel
 * against another on the same operands (e.g. the generic weight-gradient kernel against the three-taps one) and to sweep
 * tile / split-K plans.  Kept in a header of their own so that the public header documents only what a caller of the
 * reference's libs.models / libs.ops path needs. */
#ifndef PHNET_HIP_TUNING_H
#define PHNET_HIP_TUNING_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* force tile/split-K of the next phnet_conv2d_fwd / _dgrad calls; bm = 0 -> heuristic */
int phnet_tune_force_conv_tile(int32_t bm, int32_t bn, int32_t splits);
int phnet_tune_force_k_tile(int32_t k_tile);   /* 0 = heuristic, else 16 | 32 | 64; -1 / -2: uniform-tap kernel variant off / on;
                                                  -5 / -6: three-taps 3x3 stride-1 forward / dgrad kernel off / on;
                                                  -300 / -301: tall-tile kernel of the many-row Linear layers (csrc/linrows.hip) off /
                                                  on for the shape class it was measured faster at; -302: on for every Linear-shaped
                                                  phnet_conv2d_fwd / _dgrad launch without addend / statistics that it can run (arithmetic
                                                  mode 3, K % 16 == 0, operands below 2 GB), whatever the rows, columns, depth, forced tile
                                                  or forced K tile - how tests reach it at small shapes;
                                                  -400 / -401: arithmetic mode 4 without (default) / with mode 3's split-K plan */
int phnet_tune_wgrad(int32_t allow_bm128, int32_t target_blocks);   /* wgrad tile / split-K policy; bits of the first argument:
                                                                        1 = no few-rows Linear kernel, 3 = no three-taps 3x3 kernel,
                                                                        4 = its 32-pixel steps, 5 = no producer / consumer variant
                                                                        (csrc/wgrad3s.hip), 6 = no 128 x 128 producer / consumer Linear
                                                                        kernel (csrc/wgrad1s.hip); a NEGATIVE second argument sets the
                                                                        three-taps kernel's workgroup target (default 256) */
/* arithmetic of the GEMM kernels: 3 = exact three-term bf16 split staged in LDS (library default), 0 = f32-input MFMA,
 * 1 = two-term bf16 split in registers (3 MFMAs per product, ~2^-16 per product), 2 = three-term split in registers,
 * 4 = bf16 inference arithmetic (Python name "bf16").  The rule of mode 4:
 *   - a forward GEMM rounds every element of both operands to bf16, round to nearest even, exactly once, while the tile is staged
 *     (weights of the packed 3x3 kernel: while they are packed).  The operands are the f32 activations the launch was given and the
 *     f32 weights the fp32 path would have used (after the eval-mode BatchNorm fold); the conversion is the one the exact split
 *     uses for its `hi` term;
 *   - products are exact in f32 (8 + 8 mantissa bits) and are summed in the f32 accumulators of v_mfma_f32_32x32x16_bf16, ONE MFMA
 *     per 16-deep product (mode 3: six);
 *   - bias, addend (residual), ReLU, split-K partial sums and the statistics rows stay f32, exactly as in mode 3; outputs are f32;
 *   - forward only: phnet_conv2d_dgrad, phnet_conv2d_wgrad, phnet_linear_bwd and the backward queries (phnet_conv2d_kernel with
 *     dgrad = 1, phnet_conv2d_wgrad_kernel, phnet_linear_bwd_kernel) return PHNET_ERR_ARG; phnet_conv3p_fwd takes the one-plane image
 *     of phnet_conv3p_pack_bf16, which has no data-gradient packing;
 *   - no forward launch runs silently in another arithmetic: every forward kernel a shape can be dispatched to in mode 4 is a
 *     mode-4 instantiation (conv_igemm_kernel<..., 4, ...>, conv3p_bf16_kernel, linrows_bf16_kernel); the three-taps kernel, which has
 *     none, is not selected.
 *   - mode 4 does not split K on its own (a forced split count is honoured; phnet_tune_force_k_tile(-401) gives it mode 3's split
 *     plan back): unsplit, an output's bits do not depend on the batch it was computed in, so a stream step equals the clip.
 * Kernels that do not read the mode (dynamic head, row chains, towers, attention, gate) keep their arithmetic.
 * Modes 3 and 4 run with a 4-tile register ring (pf), the others with 1. */
int phnet_tune_mma(int32_t mode);
/* packed-weight 3x3 kernel: workgroups a launch is topped up to by split-K (default 512); -1 / -2: 128-column tiles off / on */
int phnet_conv3p_tune(int32_t target_workgroups);
/* routing gate's depth-wise stack: 1 = one wavefront per plane (csrc/gate_wave.hip, default where C = 64, P = 36), 0 = the generic
 * one-workgroup-per-plane kernels (csrc/gate.hip) */
int phnet_tune_gate_wave(int32_t on);
/* per-anchor products of the dynamic head: 1 = matrix-pipe kernels, one wavefront per anchor (csrc/dyn_mfma.hip, default where they
 * apply; forward: one wavefront per anchor AND 16-row fragment, backward: four per anchor), 3 = the one-wavefront-per-anchor forms of both,
 * 0 = the LDS / FMA kernels of csrc/dynhead.hip */
int phnet_tune_dyn_mfma(int32_t on);
int phnet_tune_reset(void);     /* every switch above back to its default */
int phnet_tune_mma_get(void);   /* the current phnet_tune_mma mode */

#ifdef __cplusplus
}
#endif
#endif
