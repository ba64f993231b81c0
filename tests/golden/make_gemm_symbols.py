"""Writes tests/golden/gemm_symbols_default.json: the kernel symbol and split-K factor that phnet_amd.hip_ops reports to the
kernel timer for a fixed list of GEMM shapes, in the default tuning.  No GPU is needed: the wrappers are walked with `meta`
tensors and a `_timed_launch` that evaluates the symbol and skips the launch.

The committed fixture was written by this script at the last commit whose hip_ops.py still spelled the symbols in Python
(a hand-kept copy of the C++ dispatch heuristics); tests/test_dispatch_cpu.py holds the library's
own phnet_*_kernel queries to it.  Run today it records what those queries answer.

    python tests/golden/make_gemm_symbols.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import torch  # noqa: E402

from phnet_amd import build, hip_ops as K  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_symbols_default.json")


def shape_list():
    """(N, Hi, Wi, Ci, Co, R, stride, pad): the bench_conv.py rows at 1 and 8 clips, then the trunk / neck layers they lack."""
    argv, sys.argv = sys.argv, sys.argv[:1]
    try:
        from bench_conv import SHAPES
    finally:
        sys.argv = argv
    rows = [(n * clips, hi, wi, ci, co, r, st, pad) for clips in (1, 8) for _, n, hi, wi, ci, co, r, st, pad in SHAPES]
    for ci, co, hi, wi in ((64, 128, 80, 200), (128, 256, 40, 100), (256, 512, 20, 50)):     # ResNet-34 stage entries at 5 x 320 x 800
        rows.append((5, hi, wi, ci, co, 3, 2, 1))                                            # 3x3 / stride 2
        rows.append((5, hi, wi, ci, co, 1, 2, 0))                                            # 1x1 / stride 2 down-sample
    for ci, hi, wi in ((128, 40, 100), (256, 20, 50), (512, 10, 25)):                        # FPN: 1x1 lateral, 3x3 output
        rows.append((5, hi, wi, ci, 64, 1, 1, 0))
        rows.append((5, hi, wi, 64, 64, 3, 1, 1))
    return rows


def main():
    build.build(verbose=False)
    seen = {}

    def timed_launch(sym_fn, flops, launch, shape=None, nbytes=None):
        seen["name"], seen["splits"] = sym_fn()

    def workspace(nbytes, device, slot=0):
        if slot == 0:
            seen["ws_bytes"] = int(nbytes)

    K._timed_launch, K.workspace, K._req = timed_launch, workspace, (lambda t, *a, **k: t)
    meta = lambda *s: torch.empty(s, device="meta")     # noqa: E731
    entries = []

    def record(op, args, call):
        seen.clear()
        call()
        entries.append({"op": op, "args": dict(args, ws_bytes=seen.get("ws_bytes", 0)) if not op.startswith("linear") else args,
                        "name": seen["name"], "splits": int(seen["splits"])})

    for n, hi, wi, ci, co, r, st, pad in shape_list():
        ho, wo = K.conv_out_hw(hi, wi, r, r, st, pad)
        conv = dict(N=n, Hi=hi, Wi=wi, Ci=ci, Co=co, R=r, S=r, stride=st, pad=pad)
        x, w, dy = meta(n, hi, wi, ci), meta(co, r, r, ci), meta(n, ho, wo, co)
        record("fwd", conv, lambda: K.conv2d_fwd(x, w, None, st, pad))
        record("dgrad", conv, lambda: K.conv2d_dgrad(dy, w, (hi, wi), st, pad))
        record("wgrad", conv, lambda: K.conv2d_wgrad(dy, x, w.shape, st, pad))
        record("wgrad_dbias", conv, lambda: K.conv2d_wgrad(dy, x, w.shape, st, pad, dbias=meta(co)))
        m = n * hi * wi
        if r == 3 and st == 1:
            if K.conv3p_applies(m, ci, co):
                record("conv3p_fwd", dict(M=m, Ca=ci, Nn=co), lambda: K.conv3p(x, None, co))
            if K.conv3p_applies(m, co, ci):
                record("conv3p_dgrad", dict(M=m, Ca=co, Nn=ci), lambda: K.conv3p(dy, None, ci, dgrad=True))
        if r == 1 and hi == 1 and wi == 1 and K.linear_bwd_fusable(n, ci, co):
            lin = dict(M=n, K=ci, N=co)
            record("linear_bwd", lin, lambda: K.linear_bwd(meta(n, co), meta(n, ci), meta(co, ci), meta(co, ci), None, False))
            record("linear_bwd_relu", lin, lambda: K.linear_bwd(meta(n, co), meta(n, ci), meta(co, ci), meta(co, ci), None, False,
                                                               relu_y=meta(n, co)))
    with open(OUT, "w") as f:
        json.dump({"default": entries, "mirror_was_wrong": []}, f, indent=0)
        f.write("\n")
    print(f"{len(entries)} entries -> {OUT}")


if __name__ == "__main__":
    main()
