// The process-global tuning struct (csrc/tuning.h) and the setters of include/phnet_hip_tuning.h: plain field writes, no device work.
#include "common.h"
#include "tuning.h"

Tuning& tuning() { static Tuning t; return t; }

PHNET_API int phnet_tune_reset(void) { tuning() = Tuning{}; return PHNET_OK; }
PHNET_API int phnet_tune_mma_get(void) { return tuning().mma_mode; }

// force the tile (64 | 128 each) and split-K factor of the next phnet_conv2d_fwd / _dgrad calls; bm = 0 restores the heuristic
PHNET_API int phnet_tune_force_conv_tile(int32_t bm, int32_t bn, int32_t splits)
{
    if (bm != 0 && !((bm == 64 || bm == 128) && (bn == 64 || bn == 128))) return PHNET_ERR_ARG;
    Tuning& t = tuning();
    t.force_bm = bm; t.force_bn = bn; t.force_splits = splits;
    return PHNET_OK;
}

PHNET_API int phnet_tune_force_k_tile(int32_t kt)
{
    Tuning& t = tuning();
    if (kt == -1 || kt == -2) { t.uniform_tap = kt == -2; return PHNET_OK; }
    if (kt == -5 || kt == -6) { t.taps3 = kt == -6; return PHNET_OK; }
    if (kt == -32 || kt == -64) { t.deep_kt3 = -kt; return PHNET_OK; }
    if (kt == -101 || kt == -102 || kt == -104) { t.pf = -kt - 100; return PHNET_OK; }
    if (kt == -200 || kt == -201) { t.buf_loads = -kt - 200; return PHNET_OK; }
    if (kt <= -300 && kt >= -302) { t.linrows = -kt - 300; return PHNET_OK; }
    if (kt == -400 || kt == -401) { t.bf16_splitk = -kt - 400; return PHNET_OK; }
    if (kt != 0 && kt != 16 && kt != 32 && kt != 64) return PHNET_ERR_ARG;
    t.force_kt = kt;
    return PHNET_OK;
}

PHNET_API int phnet_tune_wgrad(int32_t allow_bm128, int32_t target_blocks)
{
    if (target_blocks == 0 || target_blocks < -1024) return PHNET_ERR_ARG;
    Tuning& t = tuning();
    t.wgrad_bm128 = allow_bm128 & 1; t.wgrad_smallp = !(allow_bm128 & 2); t.wgrad_bkw = (allow_bm128 & 4) ? 32 : 16;
    t.wgrad3 = !(allow_bm128 & 8); t.wgrad3_bkw = (allow_bm128 & 16) ? 32 : 16;
    t.wgrad3s = !(allow_bm128 & 32); t.wgrad1s = !(allow_bm128 & 64);
    (target_blocks < 0 ? t.wgrad3_target : t.wgrad_target) = target_blocks < 0 ? -target_blocks : target_blocks;
    return PHNET_OK;
}

PHNET_API int phnet_tune_mma(int32_t mode)
{
    if (mode < 0 || mode > 4) return PHNET_ERR_ARG;
    tuning().mma_mode = mode;
    tuning().pf = (mode == 3 || mode == 4) ? 4 : 1;            // the staged loops (exact split, bf16 inference) run with a 4-tile register ring
    return PHNET_OK;
}

PHNET_API int phnet_conv3p_tune(int32_t target_workgroups)
{
    if (target_workgroups == -1 || target_workgroups == -2) { tuning().p3_wide = target_workgroups == -2; return PHNET_OK; }
    if (target_workgroups < 1) return PHNET_ERR_ARG;
    tuning().p3_target = target_workgroups;
    return PHNET_OK;
}

PHNET_API int phnet_tune_gate_wave(int32_t on) { tuning().gate_wave = on != 0; return PHNET_OK; }
PHNET_API int phnet_tune_dyn_mfma(int32_t on) { tuning().dyn_mfma = (on & 1) != 0; tuning().dyn_rows = !(on & 2); return PHNET_OK; }
