// Internal (not part of the C-ABI): every benchmark / A-B switch of the library in one process-global struct.  Only the setters of
// include/phnet_hip_tuning.h (csrc/tuning.hip) write it; the conv / Linear / gate / dynamic-head entry points read it when they pick
// a kernel.  Not thread-safe, and it must not change while a step is being captured into a hipGraph.
#pragma once

struct Tuning {
    // ---- arithmetic and operand path of the GEMM kernels (conv.hip, conv_wgrad.hip, linear_bwd.hip) ----
    int mma_mode = 3;            // 3: exact 3-term bf16 split at staging; 0: f32-input MFMA; 1 / 2: bf16 splits in registers; 4: bf16 inference arithmetic, forward only (phnet_tune_mma)
    int pf = 4;                  // register prefetch depth in K tiles (phnet_tune_mma sets 4 in modes 3 and 4, else 1; phnet_tune_force_k_tile(-101 / -102 / -104))
    int buf_loads = 1;           // buffer-load operand path where it applies (phnet_tune_force_k_tile(-200 / -201))
    int uniform_tap = 1;         // uniform-tap kernel variant (phnet_tune_force_k_tile(-1 / -2) = off / on)
    int taps3 = 1;               // three-taps 3x3 / stride-1 forward / dgrad kernel (phnet_tune_force_k_tile(-5 / -6) = off / on)
    int linrows = 1;             // tall-tile producer / consumer kernel for the many-row Linear layers (linrows.hip; phnet_tune_force_k_tile(-300 / -301) = off / on;
                                 // -302 = 2: for EVERY Linear launch without addend / statistics the kernel can run, whatever its size and the forced plan)
    int bf16_splitk = 0;         // arithmetic mode 4 takes mode 3's split-K plan (phnet_tune_force_k_tile(-400 / -401) = off / on).  Off: mode 4 never
                                 // splits K on its own, so that an output's bits do not depend on the batch size (DESIGN.md "bf16 inference")
    int deep_kt3 = 64;           // K tile of the few-rows GEMMs in mode 3 (phnet_tune_force_k_tile(-32 / -64))
    // ---- forced forward / dgrad plan (0 = heuristic) ----
    int force_bm = 0, force_bn = 0, force_splits = 0;       // phnet_tune_force_conv_tile
    int force_kt = 0;                                       // phnet_tune_force_k_tile(16 | 32 | 64)
    // ---- weight gradient (conv_wgrad.hip; phnet_tune_wgrad: bits of its first argument, workgroup targets in its second) ----
    int wgrad_bm128 = 1;         // bit 0: 128-row tiles of the generic kernel where they win
    int wgrad_smallp = 1;        // bit 1 switches the few-rows Linear kernels (weight gradient and fused backward) off
    int wgrad_bkw = 16;          // bit 2: 32 pixels per K step of the generic kernel in mode 3
    int wgrad3 = 1;              // bit 3 switches the three-taps 3x3 kernel off
    int wgrad3_bkw = 16;         // bit 4: its 32-pixel steps
    int wgrad3s = 1;             // bit 5 switches its producer / consumer variant (wgrad3s.hip) off
    int wgrad1s = 1;             // bit 6 switches the 128 x 128 producer / consumer kernel for many-row Linear layers (wgrad1s.hip) off
    int wgrad_target = 768;      // workgroups the generic kernel is split up to (positive second argument)
    int wgrad3_target = 256;     // the same for the three-taps kernel (negative second argument)
    int smallp_max_tiles = 400;  // few-rows kernels up to this many output tiles (measured: 64 -> 400 saves 0.75 ms per step, 1300 nothing more)
    // ---- packed-weight 3x3 kernel (conv3p.hip; phnet_conv3p_tune) ----
    int p3_target = 512;         // workgroups a launch is topped up to by split-K: two per CU, evenly
    int p3_wide = 1;             // 128-column workgroup tile (64 x 64 per wave) where the output has >= 128 channels (-1 / -2 = off / on)
    // ---- routing gate and dynamic head ----
    int gate_wave = 1;           // wave-per-plane gate kernels (gate_wave.hip) where they apply (phnet_tune_gate_wave)
    int dyn_mfma = 1;            // matrix-pipe dynamic-head kernels (dyn_mfma.hip) where they apply (phnet_tune_dyn_mfma bit 0)
    int dyn_rows = 1;            // their forward with one wavefront per (anchor, row fragment), backward with four per anchor (bit 1 = off)
};

Tuning& tuning();
